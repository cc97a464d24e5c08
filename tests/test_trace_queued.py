"""Every production k_trace traversal against the exhaustive reference, ray by ray.

yafaray_amd_traceQueued (Interface.trace_queued) builds the queues, counters and launch parameters a render
hands yafamd_launch_trace, so the kernel that runs is the one a render of the scene launches under the same
environment: the LDS-resident BVH4 (traverse4) with and without the spill column and statistics, the
LDS-resident BVH2, the plain loop over a BVH2 in global memory, traceRefill4 (BVH4 in global memory, LDS top
treelet) and traceRefill8 (the quantised BVH8), and the closest-only / shadow-only launches of the overlapped
schedule.  The rays are the classes of tests/raylib.py; the reference is the oracle's loop over every triangle
(validated against the oracle's own BVH in test_trace_exhaustive_cpu.py).  In-envelope classes are asserted
with no ray left out and no tolerance: primitive, t bits, occlusion, untouched no-ray entries, ray counts,
and independence of the segment count.

The far_k classes (origins 10^k scene extents away) measure where culling stops being safe; see
profiles/trace_ray_parity.md and DESIGN.md §3 for the counts.
"""
import numpy as np
import pytest

import raylib
from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

_HOST = {"YAFARAY_AMD_BVH_BUILD": "host", "YAFARAY_AMD_TRACE": "bvh"}
_GPU = {"YAFARAY_AMD_BVH_BUILD": "gpu", "YAFARAY_AMD_TRACE": "bvh"}
# name: (environment, scene_in_lds, bvh_width, trace statistics, plain loop (takes `part`))
VARIANTS = {
    "lds-bvh4": (dict(_HOST), 1, 4, True, True),
    "lds-bvh4-nostats": (dict(_HOST), 1, 4, False, True),
    "lds-bvh4-spill": (dict(_HOST, YAFARAY_AMD_LDS_STACK="4"), 1, 4, True, True),
    "lds-bvh2": (dict(_HOST, YAFARAY_AMD_BVH_WIDTH="2"), 1, 2, True, True),
    "global-bvh2": (dict(_HOST, YAFARAY_AMD_BVH_WIDTH="2", YAFARAY_AMD_SCENE_LDS="0"), 0, 2, True, True),
    "global-bvh4": (dict(_HOST, YAFARAY_AMD_SCENE_LDS="0"), 0, 4, True, False),
    "global-bvh4-nostats": (dict(_HOST, YAFARAY_AMD_SCENE_LDS="0"), 0, 4, False, False),
    "global-bvh4-top0": (dict(_HOST, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_LDS_TOP="0"), 0, 4, True, False),
    "global-bvh4-top1": (dict(_HOST, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_LDS_TOP="1"), 0, 4, True, False),
    "global-bvh4-spill": (dict(_HOST, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_LDS_STACK="4"), 0, 4, True, False),
    "gpu-build-global": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="0"), 0, 4, True, False),
    "bvh8-global": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="1"), 0, 8, True, False),
    "bvh8-global-nostats": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="1"), 0, 8, False, False),
    "bvh8-global-top0": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="1", YAFARAY_AMD_LDS_TOP8="0"), 0, 8, True, False),
    "bvh8-global-spill": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="1", YAFARAY_AMD_LDS_STACK="4"), 0, 8, True, False),
    "bvh8-global-top0-spill": (dict(_GPU, YAFARAY_AMD_SCENE_LDS="0", YAFARAY_AMD_BVH8="1", YAFARAY_AMD_LDS_TOP8="0",
                                    YAFARAY_AMD_LDS_STACK="4"), 0, 8, True, False),
}
_ENV_KEYS = sorted({k for v in VARIANTS.values() for k in v[0]})
T0, P0, O0 = np.float32(-7.0), -7, -7      # sentinels of entries the kernel must not write
FAR_K_CLEAN = (1, 2)                        # far_k classes without a mismatch on any variant and scene (measured: profiles/trace_ray_parity.md)
NO_RAY_EVERY = 53                           # a no-ray entry before every 53rd closest ray


def open_variant(product, monkeypatch, variant, spec):
    """The scene under a variant's environment; skips the pair when a render of it would launch another
    kernel family than the variant names (stats(): scene_in_lds, bvh_width)."""
    env, in_lds, width, stats_on, _ = VARIANTS[variant]
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.L.yafaray_amd_setTraceStats(yi.h, 1 if stats_on else 0)
    # (an empty request builds the accelerator and publishes what a launch traverses; no render has run)
    yi.trace_queued(np.zeros((0, 8), np.float32), np.zeros((0, 8), np.float32), n_seg=1)
    st = yi.stats()
    if (st["scene_in_lds"], st["bvh_width"]) != (in_lds, width):
        yi.close()
        pytest.skip(f"a render of this scene launches scene_in_lds={st['scene_in_lds']} bvh_width={st['bvh_width']}, not {variant}")
    return yi, st


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
    exp_t = np.insert(t, at, T0)
    exp_prim = np.insert(prim, at, P0)
    return closest, cl, exp_t, exp_prim, is_ray, occ


def check_closest(t, prim, exp_t, exp_prim, is_ray, what):
    bad = np.flatnonzero(prim != exp_prim)
    assert len(bad) == 0, f"{what}: {len(bad)} primitive mismatches, first entries {bad[:8]}: got {prim[bad[:8]]} expected {exp_prim[bad[:8]]}"
    hit = is_ray & (exp_prim >= 0)
    bad = np.flatnonzero(t[hit].view(np.uint32) != exp_t[hit].view(np.uint32))
    assert len(bad) == 0, f"{what}: {len(bad)} hits with other t bits"
    assert np.array_equal(t[~is_ray].view(np.uint32), np.full((~is_ray).sum(), T0).view(np.uint32)), f"{what}: a no-ray entry was written"


@pytest.mark.parametrize("scene", list(raylib.SCENES))
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_queued_trace_equals_exhaustive(product, oracle_built, monkeypatch, variant, scene):
    spec, rays, ref = raylib.scene_rays(scene, oracle_built)
    closest, shadow, exp_t, exp_prim, is_ray, exp_occ = queue_inputs(rays, ref)
    yi, st = open_variant(product, monkeypatch, variant, spec)
    n_real = int(is_ray.sum())
    first = None
    for n_seg in (1, 3, None):
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        what = f"{variant} {scene} n_seg={n_seg}"
        check_closest(t, prim, exp_t, exp_prim, is_ray, what)
        bad = np.flatnonzero(occ != exp_occ)
        assert len(bad) == 0, f"{what}: {len(bad)} occlusion mismatches, first rays {bad[:8]}: got {occ[bad[:8]]}"
        assert (nc, ns) == (n_real, len(shadow)), f"{what}: the statistics count {nc} closest / {ns} shadow rays of {n_real} / {len(shadow)}"
        # (independent of the segment count: t of misses included)
        if first is None:
            first = (t, prim, occ)
        else:
            assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim) and np.array_equal(first[2], occ), what
    print(f"{variant} {scene}: scene_in_lds={st['scene_in_lds']} bvh_width={st['bvh_width']} trace_grid={st['trace_grid']} "
          f"segments={st['shade_grid']} stack_depth={st['stack_depth']} rays {n_real} + {len(shadow)}")
    if VARIANTS[variant][4]:
        # the launches of the overlapped schedule: each traces its ray kind as the full launch does and leaves the other alone
        for n_seg in (3, None):
            t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="closest", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
            assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim)
            assert (occ == O0).all() and (nc, ns) == (n_real, 0)
            t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="shadow", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
            assert np.array_equal(occ, first[2])
            assert (prim == P0).all() and (t == T0).all() and (nc, ns) == (0, len(shadow))
    # outside the envelope: origins 10^k extents away.  Asserted where every variant was measured clean
    # (FAR_K_CLEAN); beyond, culling loses hits and the counts are reported only.
    far = raylib.far_rays(scene, oracle_built)
    for k in raylib.FAR_K:
        r, ft, fprim, focc = far[k]
        t, prim, occ, _, _ = yi.trace_queued(r, r, n_seg=None)
        hit = fprim >= 0
        bad = int((prim != fprim).sum()) + int((t[hit].view(np.uint32) != ft[hit].view(np.uint32)).sum()) + int((occ != focc).sum())
        print(f"{variant} {scene}: far_{k}: {int((prim != fprim).sum())} primitive ({int(((prim < 0) & hit).sum())} hits lost), "
              f"{int((occ != focc).sum())} occlusion mismatches of {len(r)} rays")
        if k in FAR_K_CLEAN:
            assert bad == 0, f"{variant} {scene}: far_{k}: {bad} mismatches"
    # the ray-level API of the earlier tests gives the same on the control class
    g = rays["generic"]
    t, prim, occ, _, _ = yi.trace_queued(g, g, n_seg=3)
    t1, prim1 = yi.trace_closest(g)
    assert np.array_equal(prim, prim1)
    assert np.array_equal(t[prim >= 0].view(np.uint32), t1[prim >= 0].view(np.uint32))
    assert np.array_equal(occ, yi.trace_shadow(g))
    yi.close()


def test_queued_trace_refuses_bad_requests(product, monkeypatch):
    """No launch with n_seg = 0, a segment count above the trace grid, an unknown part, a closest-only launch
    of a refill loop, or a scene without geometry."""
    spec = raylib.SCENES["cornell"]()
    g = raylib.generic(spec, 64)
    yi, st = open_variant(product, monkeypatch, "lds-bvh4", spec)
    for n_seg in (0, -1, st["trace_grid"] + 1):
        with pytest.raises(RuntimeError):
            yi.trace_queued(g, g, n_seg=n_seg)
    assert not yi.L.yafaray_amd_traceQueued(yi.h, None, 0, None, 0, 1, 3, None, None, None, None)
    t, prim, occ, nc, ns = yi.trace_queued(g[:0], g[:0], n_seg=3)      # nothing to trace is not an error
    assert (len(t), len(occ), nc, ns) == (0, 0, 0, 0)
    yi.close()
    yi, st = open_variant(product, monkeypatch, "global-bvh4", spec)
    with pytest.raises(RuntimeError):
        yi.trace_queued(g, g, n_seg=3, part="closest")
    yi.close()
    yi = product.Interface()
    assert not yi.L.yafaray_amd_traceQueued(yi.h, None, 0, None, 0, 1, 0, None, None, None, None)
    yi.close()
