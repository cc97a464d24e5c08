"""The overlapped schedule (YAFARAY_AMD_OVERLAP=1: the closest rays of iteration it + 1 traced on a side
stream beside k_nee(it), k_trace split by ray kind, k_nee grids smaller than the segment count) and the
conditional pwo record.  Neither may change a result: every case compares the film as uint32 bits, the
weights and the ray / request counts between the serial schedule and the overlapped one; one case per
subject also compares with the CPU oracle (<= 4 ULP, as test_gpu_parity.py does).

Shapes are the small ones at which the schedule can go wrong: mostly empty queue segments with a ragged
last group, several chunks, two renders on one Interface, workgroups that walk several segments,
statistics frames, ineligible renders, and two device-group members on one GPU."""
import dataclasses
import os

import numpy as np
import pytest

from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "overlap_pwo_parent.npz")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def render(product, spec, chunk_slots=None, trace_stats=None, profile=False, members=None, devices=None, renders=1):
    """[(rgba, weights, stats)] of `renders` renders on one Interface; a profiled render's stats carry
    "kernel_times" (k_nee's items = the NEE requests served)."""
    yi = product.Interface()
    scenes.apply(spec, yi)
    if members is not None:
        yi.set_device_group(members, devices)
    if chunk_slots:
        yi.L.yafaray_amd_setChunkSlots(yi.h, int(chunk_slots))
    if trace_stats is not None:
        yi.L.yafaray_amd_setTraceStats(yi.h, 1 if trace_stats else 0)
    if profile:
        yi.L.yafaray_amd_setProfileKernels(yi.h, 1)
    out = []
    for _ in range(renders):
        yi.render()
        rgba, w = yi.film()
        st = yi.stats()
        if profile:
            st["kernel_times"] = yi.kernel_times()
        out.append((rgba.copy(), w.copy(), st))
    yi.close()
    return out


def assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples")):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert np.array_equal(_bits(wa), _bits(wb)), f"{(wa != wb).sum()} weights differ"
    diff = _bits(ra) != _bits(rb)
    assert not diff.any(), f"{diff.sum()} film values differ, first at {np.argwhere(diff)[0]}"
    for k in counters:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def ragged(rr):
    # 9,045 samples: 35 full groups of 256 and one of 85; most of the n_seg segments stay empty
    return scenes.cornell(67, 45, spp=3, bounces=6, rr=rr)


@pytest.mark.parametrize("profile", [False, True])
@pytest.mark.parametrize("rr", [False, True])
def test_overlap_equals_serial_ragged(product, monkeypatch, rr, profile):
    """Mostly empty segments and a partial one, Russian roulette off and on; the profiled renders also
    compare the NEE requests k_nee served, and show that the overlapped schedule really ran: every
    iteration but the first and the last launches k_trace twice."""
    spec = ragged(rr)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    a = render(product, spec, profile=profile)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    b = render(product, spec, profile=profile)[0]
    assert_same(a, b)
    assert a[2]["closest_rays"] > 0 and a[2]["shadow_rays"] > 0
    if profile:
        ka, kb = a[2]["kernel_times"], b[2]["kernel_times"]
        assert ka["k_nee"]["items"] == kb["k_nee"]["items"] > 0
        assert ka["k_nee"]["launches"] == kb["k_nee"]["launches"]
        assert ka["k_shade"]["launches"] == kb["k_shade"]["launches"]
        # one split k_trace per k_nee that has a next iteration (all but the last)
        assert kb["k_trace"]["launches"] == ka["k_trace"]["launches"] + ka["k_nee"]["launches"] - 1


def test_overlap_matches_oracle(product, oracle_built, monkeypatch):
    spec = ragged(False)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    rgba, w, st = render(product, spec)[0]
    orgba, ow, octr = oracle_built.OracleScene(spec, threads=8).render()
    assert np.array_equal(_bits(w), _bits(ow))
    d = ulp_diff(rgba, orgba)
    assert d.max() <= 4, f"{(d > 4).sum()} values > 4 ULP, max {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    assert st["closest_rays"] == octr[0]


def test_overlap_several_chunks(product, monkeypatch):
    """38,400 samples in chunks of 12,000 slots (4 chunks, the last one short): the side stream's work of
    one chunk is finished before the next chunk reuses the queues."""
    spec = scenes.cornell(80, 60, spp=8, bounces=6, rr=True)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    one = render(product, spec)[0]
    a = render(product, spec, chunk_slots=12000)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    b = render(product, spec, chunk_slots=12000)[0]
    assert_same(a, b)
    assert_same(one, b)


def test_overlap_two_renders_on_one_interface(product, monkeypatch):
    """No stale event, counter or queue state from the previous render."""
    spec = scenes.cornell(64, 48, spp=4, bounces=6, rr=True)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    a = render(product, spec)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    b1, b2 = render(product, spec, renders=2)
    assert_same(a, b1)
    assert_same(a, b2)


@pytest.mark.parametrize("trace_mult", [1, 2])
@pytest.mark.parametrize("nee", ["half", "no-divisor", "one", "over"])
def test_overlap_nee_workgroups_walk_several_segments(product, monkeypatch, nee, trace_mult):
    """k_nee with fewer workgroups than segments (half; a count that does not divide n_seg; one workgroup
    for every segment; more than n_seg = the plain grid) and the closest part on n_seg and 2 n_seg
    workgroups: the knobs move speed only."""
    spec = ragged(True)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    a = render(product, spec)[0]
    n_seg = int(a[2]["shade_grid"])
    assert n_seg >= 4
    g = {"half": n_seg // 2, "no-divisor": n_seg // 3 + 1, "one": 1, "over": n_seg + 7}[nee]
    if nee == "no-divisor":
        while n_seg % g == 0:
            g += 1
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP_NEE_GRID", str(g))
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP_TRACE_GRID", str(trace_mult * n_seg))
    b = render(product, spec)[0]
    assert_same(a, b)


def test_overlap_trace_statistics(product, monkeypatch):
    """Statistics frames: both parts of k_trace add to node_visits / tri_tests of the same records, one
    after the other."""
    spec = ragged(True)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    a = render(product, spec, trace_stats=True)[0]
    off = render(product, spec, trace_stats=False)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP_NEE_GRID", str(int(a[2]["shade_grid"]) // 2))
    b = render(product, spec, trace_stats=True)[0]
    assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples", "node_visits", "tri_tests"))
    assert a[2]["node_visits"] > 0 and a[2]["tri_tests"] > 0
    assert_same(off, b)


INELIGIBLE = {
    # one-thread light pick: a count run, then the render (or the deferred pick's path pass)
    "two-lights": lambda: scenes.with_extra_lights(scenes.cornell(48, 36, spp=2, bounces=4, rr=False), 2),
    # photon mapping: k_gather between k_shade and k_nee
    "photon": lambda: scenes.cornell_photon(48, 36, spp=1, photons=4000, search=20, radius=0.1),
    # k_tshadow between k_trace and k_shade
    "transparent-shadows": lambda: scenes.cornell_transparent_shadows(48, 36, spp=2),
}


@pytest.mark.parametrize("case", list(INELIGIBLE))
def test_ineligible_renders_stay_serial(product, monkeypatch, case):
    """With YAFARAY_AMD_OVERLAP=1 these renders run the single-stream sequence: the same launches, the
    same film."""
    spec = INELIGIBLE[case]()
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    a = render(product, spec, profile=True)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    b = render(product, spec, profile=True)[0]
    assert_same(a, b)
    ka, kb = a[2]["kernel_times"], b[2]["kernel_times"]
    assert {k: v["launches"] for k, v in ka.items()} == {k: v["launches"] for k, v in kb.items()}
    assert ka["k_trace"]["launches"] > 0


def test_overlap_two_group_members_on_one_gpu(product, monkeypatch):
    """Two logical device-group members on GPU 0, each with its own side stream, render concurrently."""
    spec = scenes.cornell(64, 50, spp=3, bounces=5, rr=True)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    serial = render(product, spec, members=1)[0]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "1")
    one = render(product, spec, members=1)[0]
    two = render(product, spec, members=2, devices=[0, 0])[0]
    assert_same(serial, one)
    assert_same(one, two, counters=())   # (halo rows are rendered by both members: more samples and rays)


def test_default_schedule(product, monkeypatch):
    """Without YAFARAY_AMD_OVERLAP an eligible render takes the overlapped schedule (the split k_trace
    launches show in a profiled render), except for device-group members that share a GPU, which
    already run beside each other and stay serial.  The film is the same either way."""
    spec = scenes.cornell(64, 50, spp=3, bounces=5, rr=True)
    launches = lambda r: r[2]["kernel_times"]["k_trace"]["launches"]
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    serial = render(product, spec, profile=True)[0]
    serial2 = render(product, spec, profile=True, members=2, devices=[0, 0])[0]
    monkeypatch.delenv("YAFARAY_AMD_OVERLAP")
    one = render(product, spec, profile=True)[0]
    two = render(product, spec, profile=True, members=2, devices=[0, 0])[0]
    assert_same(serial, one)
    assert_same(serial2, two)
    assert_same(serial, two, counters=())
    assert launches(one) > launches(serial)
    assert launches(two) == launches(serial2)


def pwo_scene():
    """cornell_specular as a path-traced scene whose tall box is a perfect mirror over a diffuse layer
    (specular_reflect 1, no Fresnel): the material has a diffuse component, so its first hits start
    subpaths, but the diffuse layer's share of the energy is 0 and sample() draws nothing."""
    s = scenes.cornell_specular(64, 48, spp=2, integrator="pathtracing", bounces=4, raydepth=2, fresnel=False)
    mats = [dataclasses.replace(m, specular_reflect=1.0, diffuse_reflect=0.8) if m.name == "tall_mirror" else m for m in s.materials]
    return dataclasses.replace(s, materials=mats)


def test_pwo_record_only_for_unsampled_first_segments(product, oracle_built, monkeypatch):
    """k_shade keeps Pn.pwo only for first segments whose sample() drew nothing (F_SAMPLED clear).

    In this scene the camera samples whose first hit is the tall box are such entries: 13.3 % of the
    pixels' centre rays (408 of 3,072, found with the oracle's trace_closest on the CPU), plus the recursion
    tree's nodes that land on it.  They store and load the record.  The consumer `else wo = pwo`
    itself still runs for none of them, here or in any scene: a sample() that draws nothing leaves
    the direction at zero, a zero direction makes every triangle test's determinant 0, so the entry has
    no hit and ends its subpath before the branch.  The branch is covered by inspection only; what the
    test pins is that gating the record changes nothing: <= 4 ULP of the oracle, and the bits the parent
    commit rendered (tests/golden/overlap_pwo_parent.npz: its film and weights of this scene and of the
    plain Cornell box below, serial schedule)."""
    gold = np.load(GOLDEN)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", "0")
    spec = pwo_scene()
    rgba, w, st = render(product, spec)[0]
    orgba, ow, _ = oracle_built.OracleScene(spec, threads=8).render()
    assert np.array_equal(_bits(w), _bits(ow))
    d = ulp_diff(rgba, orgba)
    assert d.max() <= 4, f"{(d > 4).sum()} values > 4 ULP, max {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    assert np.array_equal(_bits(rgba), gold["mirror_rgba"]) and np.array_equal(_bits(w), gold["mirror_w"])
    # every first segment sampled (the flagship's case): no record is written or read
    rgba, w, _ = render(product, scenes.cornell(64, 48, spp=2, bounces=4, rr=True))[0]
    assert np.array_equal(_bits(rgba), gold["cornell_rgba"]) and np.array_equal(_bits(w), gold["cornell_w"])
