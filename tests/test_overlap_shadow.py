"""The early shadow part (YAFARAY_AMD_OVERLAP_SHADOW=1): under the overlapped schedule the shadow rays of
iteration it + 1 are traced right behind k_nee(it) on the render stream, beside the closest part still running
on the side stream; the render stream joins the side stream after that launch, and the early shadow part
counts into its own statistics records.  It may not change a result: every case compares the film as uint32
bits, the weights and the ray / sample counts between the serial schedule (YAFARAY_AMD_OVERLAP=0) and
YAFARAY_AMD_OVERLAP=1 with YAFARAY_AMD_OVERLAP_SHADOW=1; one case also compares with the CPU oracle (<= 4 ULP).

The shapes are those of test_overlap_schedule.py: mostly empty queue segments with a ragged last group, several
chunks, two renders on one Interface, grids that let either chain (k_nee -> shadow part, closest part) end
first, statistics frames, ineligible renders, and two device-group members on one GPU.  The serial renders are
made once per (scene, settings) and shared."""
import numpy as np
import pytest

from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

ENV = ("YAFARAY_AMD_OVERLAP", "YAFARAY_AMD_OVERLAP_SHADOW", "YAFARAY_AMD_OVERLAP_NEE_GRID", "YAFARAY_AMD_OVERLAP_TRACE_GRID",
       "YAFARAY_AMD_OVERLAP_SHADOW_GRID")


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
    "kernel_times"."""
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


def schedule(monkeypatch, overlap, shadow=None, grids=None):
    """The schedule of the renders that follow: serial (overlap 0), or overlapped with the shadow part behind
    the join (shadow 0) or beside the closest part (shadow 1); grids: nee / trace / shadow."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", str(overlap))
    if shadow is not None:
        monkeypatch.setenv("YAFARAY_AMD_OVERLAP_SHADOW", str(shadow))
    for k, v in (grids or {}).items():
        monkeypatch.setenv(f"YAFARAY_AMD_OVERLAP_{k.upper()}_GRID", str(v))


_SERIAL = {}


def serial(product, monkeypatch, key, spec, **kw):
    """The serial schedule's render of `spec` (made once per key, never modified)."""
    if key not in _SERIAL:
        schedule(monkeypatch, 0)
        _SERIAL[key] = render(product, spec, **kw)[0]
    return _SERIAL[key]


def assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples")):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert np.array_equal(_bits(wa), _bits(wb)), f"{(wa != wb).sum()} weights differ"
    diff = _bits(ra) != _bits(rb)
    assert not diff.any(), f"{diff.sum()} film values differ, first at {np.argwhere(diff)[0]}"
    for k in counters:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def launches(r):
    return {k: v["launches"] for k, v in r[2]["kernel_times"].items()}


def ragged(rr):
    # 9,045 samples: 35 full groups of 256 and one of 85; most of the n_seg segments stay empty
    return scenes.cornell(67, 45, spp=3, bounces=6, rr=rr)


@pytest.mark.parametrize("profile", [False, True])
@pytest.mark.parametrize("rr", [False, True])
def test_shadow_overlap_equals_serial_ragged(product, monkeypatch, rr, profile):
    """Mostly empty segments and a partial one, Russian roulette off and on.  The profiled renders (an event
    pair around every launch, the side stream's included) also show the launch counts of the overlapped
    schedule with the shadow part behind the join: the early shadow part moves a launch, it adds none."""
    spec = ragged(rr)
    a = serial(product, monkeypatch, ("ragged", rr, profile), spec, profile=profile)
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, profile=profile)[0]
    assert_same(a, b)
    assert a[2]["closest_rays"] > 0 and a[2]["shadow_rays"] > 0
    if profile:
        schedule(monkeypatch, 1, 0)
        c = render(product, spec, profile=profile)[0]
        assert_same(a, c)
        assert launches(b) == launches(c)
        ka, kb = a[2]["kernel_times"], b[2]["kernel_times"]
        assert ka["k_nee"]["items"] == kb["k_nee"]["items"] > 0
        # the overlapped schedule really ran: one split k_trace per k_nee that has a next iteration
        assert kb["k_trace"]["launches"] == ka["k_trace"]["launches"] + ka["k_nee"]["launches"] - 1


def test_shadow_overlap_matches_oracle(product, oracle_built, monkeypatch):
    spec = ragged(False)
    schedule(monkeypatch, 1, 1)
    rgba, w, st = render(product, spec)[0]
    orgba, ow, octr = oracle_built.OracleScene(spec, threads=8).render()
    assert np.array_equal(_bits(w), _bits(ow))
    d = ulp_diff(rgba, orgba)
    assert d.max() <= 4, f"{(d > 4).sum()} values > 4 ULP, max {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    assert st["closest_rays"] == octr[0]


def test_shadow_overlap_trace_statistics(product, monkeypatch):
    """Statistics frames: the early shadow part adds its node visits and triangle tests to its own records
    while the closest part adds to the first range; the host's sum is the serial schedule's.  A render without
    the per-visit counters on the same schedule matches too."""
    spec = ragged(True)
    a = serial(product, monkeypatch, ("ragged-stats",), spec, trace_stats=True)
    off = serial(product, monkeypatch, ("ragged", True, False), spec)
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, trace_stats=True)[0]
    assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples", "node_visits", "tri_tests"))
    assert a[2]["node_visits"] > 0 and a[2]["tri_tests"] > 0
    b_off = render(product, spec, trace_stats=False)[0]
    assert_same(off, b_off)
    assert_same(a, b_off)


@pytest.mark.parametrize("shadow_grid", ["n_seg", "default"])
@pytest.mark.parametrize("trace_mult", [1, 2])
@pytest.mark.parametrize("nee", ["one", "half", "no-divisor", "over"])
def test_shadow_overlap_either_chain_ends_first(product, monkeypatch, nee, trace_mult, shadow_grid):
    """k_nee on one workgroup (the closest part ends long before the shadow part starts) up to more than n_seg
    (the plain grid: the shadow part starts first and may end before the closest part), the closest part on
    n_seg and 2 n_seg workgroups, the shadow part on n_seg and on its default grid: the knobs move speed
    only."""
    spec = ragged(True)
    a = serial(product, monkeypatch, ("ragged", True, False), spec)
    n_seg = int(a[2]["shade_grid"])
    assert n_seg >= 4
    g = {"half": n_seg // 2, "no-divisor": n_seg // 3 + 1, "one": 1, "over": n_seg + 7}[nee]
    if nee == "no-divisor":
        while n_seg % g == 0:
            g += 1
    grids = {"nee": g, "trace": trace_mult * n_seg}
    if shadow_grid == "n_seg":
        grids["shadow"] = n_seg
    schedule(monkeypatch, 1, 1, grids)
    b = render(product, spec)[0]
    assert_same(a, b)


def test_shadow_overlap_several_chunks(product, monkeypatch):
    """38,400 samples in chunks of 12,000 slots (4 chunks, the last one short): both streams' work of one
    chunk is finished before the next chunk reuses the queues."""
    spec = scenes.cornell(80, 60, spp=8, bounces=6, rr=True)
    one = serial(product, monkeypatch, ("chunks-one",), spec)
    a = serial(product, monkeypatch, ("chunks",), spec, chunk_slots=12000)
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, chunk_slots=12000)[0]
    assert_same(a, b)
    assert_same(one, b)


def test_shadow_overlap_two_renders_on_one_interface(product, monkeypatch):
    """No stale event, statistics record, counter or queue state from the previous render."""
    spec = scenes.cornell(64, 48, spp=4, bounces=6)
    a = serial(product, monkeypatch, ("two-renders",), spec)
    schedule(monkeypatch, 1, 1)
    b1, b2 = render(product, spec, renders=2)
    assert_same(a, b1)
    assert_same(a, b2)


def test_shadow_overlap_off_reproduces_on(product, monkeypatch):
    """YAFARAY_AMD_OVERLAP_SHADOW=0 (the shadow part behind the join) against =1, statistics included."""
    spec = ragged(True)
    schedule(monkeypatch, 1, 0)
    a = render(product, spec, trace_stats=True)[0]
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, trace_stats=True)[0]
    assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples", "node_visits", "tri_tests"))
    assert b[2]["shadow_rays"] > 0 and b[2]["node_visits"] > 0


def test_shadow_overlap_with_a_spill_column(product, monkeypatch):
    """Four stack levels in LDS: where the scene's stack bound is deeper, k_trace has a spill column and the
    shadow part stays behind the join (two launches would share the columns).  Either way the result is the
    serial schedule's under the same setting."""
    spec = ragged(True)
    monkeypatch.setenv("YAFARAY_AMD_LDS_STACK", "4")
    a = serial(product, monkeypatch, ("ragged-lds4",), spec, trace_stats=True)
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, trace_stats=True)[0]
    assert_same(a, b, counters=("closest_rays", "shadow_rays", "samples", "node_visits", "tri_tests"))


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
    """With YAFARAY_AMD_OVERLAP=1 and YAFARAY_AMD_OVERLAP_SHADOW=1 these renders run the single-stream
    sequence: the same launches, the same film."""
    spec = INELIGIBLE[case]()
    a = serial(product, monkeypatch, ("ineligible", case), spec, profile=True)
    schedule(monkeypatch, 1, 1)
    b = render(product, spec, profile=True)[0]
    assert_same(a, b)
    assert launches(a) == launches(b)
    assert launches(a)["k_trace"] > 0


def test_shadow_overlap_two_group_members_on_one_gpu(product, monkeypatch):
    """Two logical device-group members on GPU 0, each with its own side stream and statistics records,
    render concurrently."""
    spec = scenes.cornell(64, 50, spp=3, bounces=5, rr=True)
    a = serial(product, monkeypatch, ("group",), spec, members=1)
    schedule(monkeypatch, 1, 1)
    one = render(product, spec, members=1)[0]
    two = render(product, spec, members=2, devices=[0, 0])[0]
    assert_same(a, one)
    assert_same(one, two, counters=())   # (halo rows are rendered by both members: more samples and rays)
