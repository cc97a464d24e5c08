"""Stage-specialised k_shade launches (YAFARAY_AMD_SHADE_STAGES, on by default): in a render of the lean path
tracer (compact records, one path per sample, no recursion tree, no one-thread light pick) the stage of every
live entry follows from the iteration, so iteration 0 launches the camera kernel (which reads no pr record and
derives the sample id from the queue address; k_camera writes no record then), iteration 1 the first-segment
kernel and the later iterations the bounce kernel.  They may not change a result: every case renders with
YAFARAY_AMD_SHADE_STAGES=0 (the kernel that reads the stage from the record) and with the default, and compares
the film as uint32 bits, the weights, the ray and sample counts and k_shade's entry count; one case also compares
with the CPU oracle (<= 4 ULP).

The profile records name what ran: "k_shade_staged" counts the stage-specialised launches among k_shade's, all
of them in an eligible render and none in an ineligible one.  A render fails when a stage-specialised kernel
meets an entry of another stage (the device guard words), so every eligible case below is also a check that
the guard stays at zero."""
import dataclasses

import numpy as np
import pytest

from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


def render(product, spec, chunk_slots=None, renders=1):
    """[(rgba, weights, stats)] of `renders` profiled renders on one Interface (stats["kernel_times"])."""
    yi = product.Interface()
    scenes.apply(spec, yi)
    if chunk_slots:
        yi.L.yafaray_amd_setChunkSlots(yi.h, int(chunk_slots))
    yi.L.yafaray_amd_setProfileKernels(yi.h, 1)
    out = []
    for _ in range(renders):
        yi.render()
        rgba, w = yi.film()
        st = yi.stats()
        st["kernel_times"] = yi.kernel_times()
        out.append((rgba.copy(), w.copy(), st))
    yi.close()
    return out


def both(product, monkeypatch, spec, **kw):
    """(generic, staged): the render with YAFARAY_AMD_SHADE_STAGES=0 and the default one."""
    monkeypatch.setenv("YAFARAY_AMD_SHADE_STAGES", "0")
    a = render(product, spec, **kw)
    monkeypatch.delenv("YAFARAY_AMD_SHADE_STAGES")
    b = render(product, spec, **kw)
    return a, b


def launches(r, kind):
    return r[2]["kernel_times"].get(kind, {}).get("launches", 0)


def assert_same(a, b, same_launches=True):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert np.array_equal(_bits(wa), _bits(wb)), f"{(wa != wb).sum()} weights differ"
    diff = _bits(ra) != _bits(rb)
    assert not diff.any(), f"{diff.sum()} film values differ, first at {np.argwhere(diff)[0]}"
    for k in ("closest_rays", "shadow_rays", "samples"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    ea, eb = sa["kernel_times"]["k_shade"], sb["kernel_times"]["k_shade"]
    assert ea["items"] == eb["items"] > 0, ("shade_entries", ea["items"], eb["items"])
    assert not same_launches or ea["launches"] == eb["launches"]


def assert_staged(a, b):
    """a ran the generic kernel only, b the stage-specialised kernels only; same results."""
    assert_same(a, b)
    assert launches(a, "k_shade_staged") == 0
    assert launches(b, "k_shade_staged") == launches(b, "k_shade") > 0


@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("grid", [2, 5, None])
@pytest.mark.parametrize("rr", [False, True])
@pytest.mark.parametrize("shape", [(17, 13, 3), (48, 36, 4)])
def test_stages_equal_generic_ragged(product, monkeypatch, shape, rr, grid, overlap):
    """663 samples (two groups of 256 and one of 151) and 6,912 (27 groups) over 2 segments (a segment holds a full
    and a partial group, which a camera workgroup of another size than 256 walks across), 5 segments (unequal
    numbers of groups) and the default grid (most segments empty), on the serial and the overlapped schedule."""
    w, h, spp = shape
    spec = scenes.cornell(w, h, spp=spp, bounces=5, rr=rr)
    if grid is not None:
        monkeypatch.setenv("YAFARAY_AMD_SHADE_GRID", str(grid))
    monkeypatch.setenv("YAFARAY_AMD_OVERLAP", str(overlap))
    (a,), (b,) = both(product, monkeypatch, spec)
    assert_staged(a, b)
    assert a[2]["shadow_rays"] > 0
    if grid is not None:
        assert a[2]["shade_grid"] == grid


def test_stages_one_sample(product, monkeypatch):
    (a,), (b,) = both(product, monkeypatch, scenes.cornell(1, 1, spp=1, bounces=4, rr=True))
    assert_staged(a, b)
    assert a[2]["samples"] == 1


@pytest.mark.parametrize("rr", [False, True])
def test_stages_tables_in_global_memory(product, monkeypatch, rr):
    """2,082 triangles: the per-primitive normals do not fit k_shade's LDS tables (the other instantiations)."""
    (a,), (b,) = both(product, monkeypatch, scenes.cornell_sphere(n=32, width=40, height=30, spp=2, bounces=4, rr=rr))
    assert_staged(a, b)
    assert a[2]["shadow_rays"] > 0


def test_stages_several_chunks_and_two_renders(product, monkeypatch):
    """9,045 samples in chunks of 4,000 slots (the last chunk short), twice on one Interface."""
    spec = scenes.cornell(67, 45, spp=3, bounces=6, rr=True)
    (one,), _ = both(product, monkeypatch, spec)
    a, b = both(product, monkeypatch, spec, chunk_slots=4000, renders=2)
    for k in range(2):
        assert_staged(a[k], b[k])
        assert_same(one, b[k], same_launches=False)   # (one chunk: a third of the launches)
    assert launches(b[0], "k_camera") == 3


@pytest.mark.parametrize("rr", [False, True])
@pytest.mark.parametrize("bounces", [0, 1, 2])
def test_stages_small_depths(product, monkeypatch, bounces, rr):
    """Depth 0, 1 and 2: the first-segment or the first bounce iteration ends every path."""
    (a,), (b,) = both(product, monkeypatch, scenes.cornell(33, 21, spp=2, bounces=bounces, rr=rr))
    assert_staged(a, b)


def test_stages_camera_sees_the_emitter(product, monkeypatch):
    """A camera below the meshlight's panel looking up at it: non-diffuse camera hits that end in iteration 0."""
    spec = scenes.cornell_meshlight(40, 30, spp=2, bounces=3).with_camera(from_=(0.0, -1.5, 0.4), to=(0.0, 0.0, 1.9), up=(0.0, -1.5, 1.4))
    (a,), (b,) = both(product, monkeypatch, spec)
    assert_staged(a, b)
    assert a[0][..., :3].max() > 1.0   # the lamp itself is on the film


@pytest.mark.parametrize("transparent", [False, True])
def test_stages_camera_sees_the_background(product, monkeypatch, transparent):
    """A wide camera sees past the box: camera rays without a hit, the constant and the transparent background."""
    spec = dataclasses.replace(scenes.cornell(40, 30, spp=2, bounces=3), background=scenes.Background((0.2, 0.3, 0.4), 1.0))
    spec = spec.with_camera(focal=0.5).with_render(bg_transp=transparent)
    (a,), (b,) = both(product, monkeypatch, spec)
    assert_staged(a, b)
    assert a[2]["closest_rays"] > 0
    corner = a[0][0, 0]
    assert corner[3] == (0.0 if transparent else 1.0)
    assert (corner[:3] == 0.0).all() if transparent else (corner[:3] > 0.0).all()


def test_stages_cropped_film_and_adaptive_passes(product, monkeypatch):
    """A cropped film (the pixel hash takes the camera pixel) and adaptive passes (sampleAt's pixel list): the
    sample id the camera kernel derives must be the one k_camera dealt."""
    spec = scenes.cornell(80, 64, spp=2, bounces=3, rr=True).with_render(width=44, height=30, xstart=9, ystart=17, aa_passes=3,
                                                                          aa_inc_samples=2, aa_threshold=0.02)
    (a,), (b,) = both(product, monkeypatch, spec)
    assert_staged(a, b)
    assert a[2]["samples"] > 44 * 30 * 2   # a pixel-list pass ran


INELIGIBLE = {
    # one-thread light pick: count runs, S.lpc_mode != 0
    "two-lights": lambda: scenes.with_extra_lights(scenes.cornell(48, 36, spp=2, bounces=4, rr=False), 2),
    # several subpaths per sample: first segments in later iterations too
    "path-samples-2": lambda: scenes.cornell(48, 36, spp=2, bounces=3, rr=False).with_render(path_samples=2),
    # surface attributes: the EXT kernel
    "textured": lambda: scenes.test01_textured(48, 48, spp=2).with_render(integrator="pathtracing", bounces=3),
    # specular recursion tree: full records, spawned nodes
    "mirror": lambda: scenes.cornell_specular(48, 36, spp=2, integrator="pathtracing", bounces=3),
}


@pytest.mark.parametrize("case", list(INELIGIBLE))
def test_ineligible_renders_take_the_generic_kernel(product, monkeypatch, case):
    (a,), (b,) = both(product, monkeypatch, INELIGIBLE[case]())
    assert_same(a, b)
    assert launches(a, "k_shade") > 0
    assert launches(a, "k_shade_staged") == 0 and launches(b, "k_shade_staged") == 0
    assert {k: v["launches"] for k, v in a[2]["kernel_times"].items()} == {k: v["launches"] for k, v in b[2]["kernel_times"].items()}


def test_general_kernels_stay_generic(product, monkeypatch):
    """YAFARAY_AMD_SHADE_LEAN=0 (the general k_shade): no stage-specialised launch, the same film."""
    spec = scenes.cornell(48, 36, spp=2, bounces=4, rr=True)
    (a,), (b,) = both(product, monkeypatch, spec)
    monkeypatch.setenv("YAFARAY_AMD_SHADE_LEAN", "0")
    (c,) = render(product, spec)
    assert_staged(a, b)
    assert_same(a, c)
    assert launches(c, "k_shade_staged") == 0


def test_stages_match_oracle(product, oracle_built, monkeypatch):
    spec = scenes.cornell(67, 45, spp=3, bounces=6, rr=False)
    monkeypatch.delenv("YAFARAY_AMD_SHADE_STAGES", raising=False)
    (b,) = render(product, spec)
    assert launches(b, "k_shade_staged") == launches(b, "k_shade") > 0
    orgba, ow, octr = oracle_built.OracleScene(spec, threads=8).render()
    assert np.array_equal(_bits(b[1]), _bits(ow))
    d = ulp_diff(b[0], orgba)
    assert d.max() <= 4, f"{(d > 4).sum()} values > 4 ULP, max {d.max()} at {np.unravel_index(d.argmax(), d.shape)}"
    assert b[2]["closest_rays"] == octr[0]
