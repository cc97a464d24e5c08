"""k_trace's flat scan (YAFARAY_AMD_TRACE_FLAT; trace.h traverseFlat) against the exhaustive reference, ray by
ray, through the launch a render of the scene uses (Interface.trace_queued), with the conventions of
test_trace_deferred.py: every in-envelope ray class of tests/raylib.py, no-ray entries mixed in, primitive, t
bits, occlusion, untouched sentinels and ray counts, no tolerance and no ray left out, for 1 / 3 / the render's own
segment count and for the closest-only / shadow-only launches; far_1 / far_2 clean.

The scan tests every leaf box of the scene in a wave-uniform loop and then the triangles of the hit leaves by
the bits of a 64-bit mask.  FLAT=1 forces it whatever the leaf count, with the per-visit statistics on and off.
Scenes: the Cornell box and its first 1 / 2 / 5 triangles, cornell-fan (50 triangles: rays crossing many leaves,
bits in both mask words), dust of 33 triangles (bit 32) and of 64 (bit 63; 64 leaves, far above the automatic
limit), cornell-fan with leaves of up to 8 triangles (a leaf of 7; the builder puts none of its leaves across
slots 31 / 32) and dust of 64 with leaves of up to 8 (a leaf of 8, and one leaf whose bits lie in both mask words:
the scan's middle loop; tests/test_flat_table.py checks on the CPU that this tree has it).

Scenes that are not eligible (65 triangles; a scene kept in global memory) run the same kernels under FLAT=1 and
FLAT=0: equal hits through trace_queued, and renders with equal films and equal node_visits / tri_tests.
"""
import numpy as np
import pytest

import raylib
from libyafaray_amd import scenes
from test_trace_deferred import FAR_K_CLEAN, O0, P0, T0, check_closest, queue_inputs
from test_trace_deferred import scene_rays as deferred_scene_rays

pytestmark = pytest.mark.gpu

_BASE = {"YAFARAY_AMD_BVH_BUILD": "host", "YAFARAY_AMD_TRACE": "bvh"}
_ENV_KEYS = ("YAFARAY_AMD_BVH_BUILD", "YAFARAY_AMD_TRACE", "YAFARAY_AMD_TRACE_DEFER", "YAFARAY_AMD_TRACE_DEFER_CAP", "YAFARAY_AMD_TRACE_FLAT",
             "YAFARAY_AMD_TRACE_FLAT_IT0", "YAFARAY_AMD_BVH_LEAF", "YAFARAY_AMD_BVH_WIDTH", "YAFARAY_AMD_SCENE_LDS", "YAFARAY_AMD_LDS_STACK",
             "YAFARAY_AMD_BVH8")

# name -> (the scene of the rays and the reference, extra settings)
CASES = {
    "cornell": ("cornell", {}),
    "cornell-1": ("cornell-1", {}),
    "cornell-2": ("cornell-2", {}),
    "cornell-5": ("cornell-5", {}),
    "cornell-fan": ("cornell-fan", {}),
    "dust-33": ("dust-33t", {}),
    "dust-64": ("dust-64t", {}),
    "cornell-fan-leaf8": ("cornell-fan", {"YAFARAY_AMD_BVH_LEAF": "8"}),
    "dust-64-leaf8": ("dust-64t", {"YAFARAY_AMD_BVH_LEAF": "8"}),
}
_DUST = {"dust-33t": 33, "dust-64t": 64, "dust-65t": 65}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def scene_rays(name, oracle):
    """raylib.scene_rays; the dust scenes of this file are made the same way (once, read-only)."""
    if name in _DUST and name not in raylib._cache:
        spec = raylib.dust(n=_DUST[name])
        assert len(spec.tris) == _DUST[name]
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
    return deferred_scene_rays(name, oracle)


def oracle_answers(rays, ref):
    """The exhaustive oracle alone answers every chosen class: one (t, primitive, occlusion) per ray, a hit's t
    finite and positive, and some class of the scene has hits and some has occluded shadow rays."""
    hits = shadows = 0
    for cls in raylib.IN_ENVELOPE:
        t, prim, occ, _ = ref[cls]
        n = len(rays[cls])
        assert n > 0 and len(t) == len(prim) == len(occ) == n, cls
        hit = prim >= 0
        assert np.isfinite(t[hit]).all() and (t[hit] > 0).all(), cls
        hits += int(hit.sum())
        shadows += int((np.asarray(occ) != 0).sum())
    assert hits > 0 and shadows > 0


def open_scene(product, monkeypatch, env, spec, stats_on):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(_BASE, **env).items():
        monkeypatch.setenv(k, v)
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.L.yafaray_amd_setTraceStats(yi.h, 1 if stats_on else 0)
    yi.trace_queued(np.zeros((0, 8), np.float32), np.zeros((0, 8), np.float32), n_seg=1)
    return yi, yi.stats()


def trace_all(yi, closest, shadow, exp_t, exp_prim, is_ray, exp_occ, what, parts=True):
    """Every launch shape against the expected hits; returns the first launch's (t, prim, occ).  parts=False: the
    launches of both ray kinds only (the refill loops of a scene in global memory have no part launches)."""
    n_real = int(is_ray.sum())
    first = None
    for n_seg in (1, 3, None):
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        w = f"{what} n_seg={n_seg}"
        check_closest(t, prim, exp_t, exp_prim, is_ray, w)
        bad = np.flatnonzero(occ != exp_occ)
        assert len(bad) == 0, f"{w}: {len(bad)} occlusion mismatches, first rays {bad[:8]}: got {occ[bad[:8]]}"
        assert (nc, ns) == (n_real, len(shadow)), f"{w}: the statistics count {nc} closest / {ns} shadow rays of {n_real} / {len(shadow)}"
        if first is None:
            first = (t, prim, occ)
        else:
            assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim) and np.array_equal(first[2], occ), w
    for n_seg in (1, 3, None) if parts else ():
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="closest", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        assert np.array_equal(first[0].view(np.uint32), t.view(np.uint32)) and np.array_equal(first[1], prim), what
        assert (occ == O0).all() and (nc, ns) == (n_real, 0), what
        t, prim, occ, nc, ns = yi.trace_queued(closest, shadow, n_seg=n_seg, part="shadow", sentinel_t=T0, sentinel_prim=P0, sentinel_occ=O0)
        assert np.array_equal(occ, first[2]), what
        assert (prim == P0).all() and (t == T0).all() and (nc, ns) == (0, len(shadow)), what
    return first


@pytest.mark.parametrize("stats_on", [True, False], ids=["stats", "nostats"])
@pytest.mark.parametrize("case", list(CASES))
def test_flat_trace_equals_exhaustive(product, oracle_built, monkeypatch, case, stats_on):
    name, extra = CASES[case]
    spec, rays, ref = scene_rays(name, oracle_built)
    oracle_answers(rays, ref)
    closest, shadow, exp_t, exp_prim, is_ray, exp_occ = queue_inputs(rays, ref)
    yi, st = open_scene(product, monkeypatch, dict(extra, YAFARAY_AMD_TRACE_FLAT="1"), spec, stats_on)
    assert (st["scene_in_lds"], st["bvh_width"]) == (1, 4), st
    trace_all(yi, closest, shadow, exp_t, exp_prim, is_ray, exp_occ, f"flat {case}")
    far = raylib.far_rays(name, oracle_built)
    for k in FAR_K_CLEAN:
        r, ft, fprim, focc = far[k]
        t, prim, occ, _, _ = yi.trace_queued(r, r, n_seg=None)
        hit = fprim >= 0
        bad = int((prim != fprim).sum()) + int((t[hit].view(np.uint32) != ft[hit].view(np.uint32)).sum()) + int((occ != focc).sum())
        assert bad == 0, f"flat {case}: far_{k}: {bad} mismatches"
    yi.close()


INELIGIBLE = {
    "dust-65": ("dust-65t", {}, 1),
    "global-memory": ("cornell", {"YAFARAY_AMD_SCENE_LDS": "0"}, 0),
}


def _render(product, monkeypatch, env, spec):
    for k in _ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in dict(_BASE, **env).items():
        monkeypatch.setenv(k, v)
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.L.yafaray_amd_setTraceStats(yi.h, 1)
    yi.render()
    rgba, w = yi.film()
    out = (rgba.copy(), w.copy(), yi.stats())
    yi.close()
    return out


@pytest.mark.parametrize("case", list(INELIGIBLE))
def test_ineligible_scenes_run_the_same_kernels(product, oracle_built, monkeypatch, case):
    name, extra, in_lds = INELIGIBLE[case]
    spec, rays, ref = scene_rays(name, oracle_built)
    oracle_answers(rays, ref)
    closest, shadow, exp_t, exp_prim, is_ray, exp_occ = queue_inputs(rays, ref)
    got = {}
    for flat in ("0", "1"):
        yi, st = open_scene(product, monkeypatch, dict(extra, YAFARAY_AMD_TRACE_FLAT=flat), spec, True)
        assert st["scene_in_lds"] == in_lds, st
        got[flat] = trace_all(yi, closest, shadow, exp_t, exp_prim, is_ray, exp_occ, f"{case} flat={flat}", parts=bool(in_lds))
        yi.close()
    (t0, p0, o0), (t1, p1, o1) = got["0"], got["1"]
    assert np.array_equal(_bits(t0), _bits(t1)) and np.array_equal(p0, p1) and np.array_equal(o0, o1)
    # renders: equal films and equal traversal counters, so the same loop ran
    ra, wa, sa = _render(product, monkeypatch, dict(extra, YAFARAY_AMD_TRACE_FLAT="0"), spec)
    rb, wb, sb = _render(product, monkeypatch, dict(extra, YAFARAY_AMD_TRACE_FLAT="1"), spec)
    assert np.array_equal(_bits(ra), _bits(rb)) and np.array_equal(_bits(wa), _bits(wb))
    for k in ("closest_rays", "shadow_rays", "samples", "node_visits", "tri_tests"):
        assert sa[k] == sb[k], (k, sa[k], sb[k])
    assert sa["node_visits"] > 0 and sa["closest_rays"] > 0
