"""k_trace's deferred leaf tests (YAFARAY_AMD_TRACE_DEFER; kernels.hip traverse4Defer) against the exhaustive
reference, ray by ray, through the launch a render of the scene uses (Interface.trace_queued, as
test_trace_queued.py).

The LDS-resident BVH4 without a spill column records the leaves a visit hits in a per-lane LDS list and tests
their triangles afterwards.  The settings: the interleaved loop (DEFER=0), the lists at their default capacity,
at the smallest capacity (a lane flushes after every visit that recorded a leaf, so box culling resumes in the
middle of a traversal) and over a tree of 8-triangle leaves with the smallest capacity (a 4-entry list then
holds up to 32 pending triangles); each with the per-visit statistics on and off.  Every in-envelope ray class of
tests/raylib.py must match with no ray left out and no tolerance: primitive, t bits, occlusion, untouched
no-ray entries, ray counts, for 1 / 3 / the render's own segment count and for the closest-only / shadow-only
launches of the overlapped schedule; the far_1 / far_2 classes are clean as in test_trace_queued.py.

(traceQueued reports ray counts only; node visits and triangle tests are compared between schedules in
test_trace_deferred_render.py.)
"""
import numpy as np
import pytest

import raylib
from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

# (the conventions of test_trace_queued.py)
T0, P0, O0 = np.float32(-7.0), -7, -7      # sentinels of entries the kernel must not write
FAR_K_CLEAN = (1, 2)
NO_RAY_EVERY = 53                           # a no-ray entry before every 53rd closest ray


def queue_inputs(rays, ref):
    """All in-envelope classes as one closest queue (no-ray entries mixed in) and one shadow queue, with the
    expected outputs: (closest, shadow, t, prim, is_ray, occluded)."""
    cl = np.concatenate([rays[c] for c in raylib.IN_ENVELOPE])
    t = np.concatenate([ref[c][0] for c in raylib.IN_ENVELOPE])
    prim = np.concatenate([ref[c][1] for c in raylib.IN_ENVELOPE])
    occ = np.concatenate([ref[c][2] for c in raylib.IN_ENVELOPE])
    at = np.arange(0, len(cl), NO_RAY_EVERY)
    closest = np.insert(cl, at, raylib.no_ray(len(at)), axis=0)
    is_ray = np.insert(np.ones(len(cl), bool), at, False)
    return closest, cl, np.insert(t, at, T0), np.insert(prim, at, P0), is_ray, occ


def check_closest(t, prim, exp_t, exp_prim, is_ray, what):
    bad = np.flatnonzero(prim != exp_prim)
    assert len(bad) == 0, f"{what}: {len(bad)} primitive mismatches, first entries {bad[:8]}: got {prim[bad[:8]]} expected {exp_prim[bad[:8]]}"
    hit = is_ray & (exp_prim >= 0)
    bad = np.flatnonzero(t[hit].view(np.uint32) != exp_t[hit].view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} hits with other t bits"
    assert np.array_equal(t[~is_ray].view(np.uint32), np.full((~is_ray).sum(), T0).view(np.uint32)), f"{what}: a no-ray entry was written"

_BASE = {"YAFARAY_AMD_BVH_BUILD": "host", "YAFARAY_AMD_TRACE": "bvh"}
SETTINGS = {
    "defer0": dict(_BASE, YAFARAY_AMD_TRACE_DEFER="0"),
    "defer1": dict(_BASE, YAFARAY_AMD_TRACE_DEFER="1"),
    "defer1-mincap": dict(_BASE, YAFARAY_AMD_TRACE_DEFER="1", YAFARAY_AMD_TRACE_DEFER_CAP="1"),
    "defer1-leaf8-mincap": dict(_BASE, YAFARAY_AMD_TRACE_DEFER="1", YAFARAY_AMD_TRACE_DEFER_CAP="1", YAFARAY_AMD_BVH_LEAF="8"),
}
_ENV_KEYS = sorted({k for v in SETTINGS.values() for k in v} |
                   {"YAFARAY_AMD_BVH_WIDTH", "YAFARAY_AMD_SCENE_LDS", "YAFARAY_AMD_LDS_STACK", "YAFARAY_AMD_BVH8"})


def cornell_fan():
    """The Cornell box plus sphere_slivers' fan of 16 triangles 1e-4 wide, without the sphere: 50 triangles,
    rays crossing many leaves."""
    sl = []
    for k in range(16):
        x = -0.8 + 0.1 * k
        sl += [(x, -0.5, 0.2), (x + 1e-4, 0.5, 0.2), (x + 2e-4, 0.0, 1.6)]
    return raylib.with_mesh(scenes.cornell(32, 32, spp=1), sl, np.arange(len(sl), dtype=np.int32).reshape(-1, 3), "slivers")


SCENES = ("cornell", "cornell-1", "cornell-2", "cornell-5", "cornell-fan", "dust")


def scene_rays(name, oracle):
    """raylib.scene_rays, with cornell-fan's rays and reference made the same way (once, read-only)."""
    if name == "cornell-fan" and name not in raylib._cache:
        spec = cornell_fan()
        assert len(spec.tris) == 50
        osc = oracle.OracleScene(spec)

        def closest(r):
            hit, prim = osc.trace_closest(r, exhaustive=True)
            return hit[:, 0].copy(), prim

        rays = raylib.ray_classes(spec, closest)
        ref = {}
        for cls, r in rays.items():
            t, prim = closest(r)
            ref[cls] = (t, prim, osc.trace_shadow(raylib.shadow_ray_of(r), exhaustive=True), osc.trace_ties(r))
            for a in ref[cls]:
                a.setflags(write=False)
            r.setflags(write=False)
        raylib._cache[name] = (spec, rays, ref)
    return raylib.scene_rays(name, oracle)


def open_scene(product, monkeypatch, setting, spec, stats_on):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in SETTINGS[setting].items():
        monkeypatch.setenv(k, v)
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.L.yafaray_amd_setTraceStats(yi.h, 1 if stats_on else 0)
    yi.trace_queued(np.zeros((0, 8), np.float32), np.zeros((0, 8), np.float32), n_seg=1)
    st = yi.stats()
    if (st["scene_in_lds"], st["bvh_width"]) != (1, 4):
        yi.close()
        pytest.skip(f"a render of this scene launches scene_in_lds={st['scene_in_lds']} bvh_width={st['bvh_width']}")
    return yi, st


@pytest.mark.parametrize("stats_on", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("scene", SCENES)
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_deferred_trace_equals_exhaustive(product, oracle_built, monkeypatch, setting, scene, stats_on):
    spec, rays, ref = scene_rays(scene, oracle_built)
    closest, shadow, exp_t, exp_prim, is_ray, exp_occ = queue_inputs(rays, ref)
    yi, st = open_scene(product, monkeypatch, setting, spec, stats_on)
    n_real = int(is_ray.sum())
    first = None
    for n_seg in (1, 3, None):
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        what = f"{setting} {scene} n_seg={n_seg}"
        check_closest(t, prim, exp_t, exp_prim, is_ray, what)
        bad = np.flatnonzero(occ != exp_occ)
        assert len(bad) == 0, f"{what}: {len(bad)} occlusion mismatches, first rays {bad[:8]}: got {occ[bad[:8]]}"
        assert (nc, ns) == (n_real, len(shadow)), f"{what}: the statistics count {nc} closest / {ns} shadow rays of {n_real} / {len(shadow)}"
        if first is None:
            first = (t, prim, occ)
        else:
            assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim) and np.array_equal(first[2], occ), what
    for n_seg in (3, None):
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="closest", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim)
        assert (occ == O0).all() and (nc, ns) == (n_real, 0)
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="shadow", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        assert np.array_equal(occ, first[2])
        assert (prim == P0).all() and (t == T0).all() and (nc, ns) == (0, len(shadow))
    far = raylib.far_rays(scene, oracle_built)
    for k in FAR_K_CLEAN:
        r, ft, fprim, focc = far[k]
        t, prim, occ, _, _ = yi.trace_queued(r, r, n_seg=None)
        hit = fprim >= 0
        bad = int((prim != fprim).sum()) + int((t[hit].view(np.uint32) != ft[hit].view(np.uint32)).sum()) + int((occ != focc).sum())
        assert bad == 0, f"{setting} {scene}: far_{k}: {bad} mismatches"
    yi.close()
