"""The ray sets of tests/raylib.py against the oracle, on the CPU: before any accelerator of the product is
compared with the exhaustive reference (a loop over every triangle, oracle/yafcpu.cc
yc_trace_*_exhaustive), the oracle's own BVH — double-precision box tests, padded boxes — must give that
reference bit for bit on every in-envelope class and scene, every class must produce hits and misses, and
the sets must contain exact t ties between primitives."""
import numpy as np
import pytest

import raylib

# rays that start on a triangle cannot hit that triangle (t below the intersection epsilon) nor one in its own
# plane: a one-triangle scene and the two coplanar triangles of the Cornell floor give on_surface no hit
_NO_HIT_POSSIBLE = {("cornell-1", "on_surface"), ("cornell-2", "on_surface")}


@pytest.mark.parametrize("scene", list(raylib.SCENES))
def test_oracle_bvh_equals_exhaustive(oracle_built, scene):
    spec, rays, ref = raylib.scene_rays(scene, oracle_built)
    osc = oracle_built.OracleScene(spec)
    total = 0
    for cls in raylib.IN_ENVELOPE:
        r = rays[cls]
        t, prim, occ, ties = ref[cls]
        hit = prim >= 0
        n_tie = int((ties >= 2).sum())
        print(f"{scene:24s} {cls:11s} rays {len(r):5d} hits {int(hit.sum()):5d} ties {n_tie:4d} occluded {int(occ.sum()):5d}")
        total += len(r)
        assert 0 < len(r) <= raylib.MAX_PER_CLASS
        bh, bprim = osc.trace_closest(r)
        assert np.array_equal(bprim, prim), f"{cls}: {(bprim != prim).sum()} primitive mismatches, first at ray {np.flatnonzero(bprim != prim)[:5]}"
        assert np.array_equal(bh[hit, 0].view(np.uint32), t[hit].view(np.uint32)), cls
        assert np.array_equal(osc.trace_shadow(raylib.shadow_ray_of(r)), occ), cls
        if (scene, cls) in _NO_HIT_POSSIBLE:
            assert not hit.any() and not occ.any()
        else:
            assert hit.any(), f"{cls}: no hits"
            assert occ.any(), f"{cls}: no shadow ray occluded"
        assert not hit.all(), f"{cls}: no misses"
        assert not occ.all(), f"{cls}: every shadow ray occluded"
        assert ((ties >= 1) == hit).all()
    assert total <= 25000


def test_cornell_rays_contain_exact_ties(oracle_built):
    """Exact t ties between different primitives (the tie rule: the lower index wins) occur in the Cornell
    box's vertex and edge classes."""
    _, rays, ref = raylib.scene_rays("cornell", oracle_built)
    n = {cls: int((ref[cls][3] >= 2).sum()) for cls in raylib.IN_ENVELOPE}
    print("cornell exact ties per class:", n)
    assert n["vertex"] > 0 and n["edge"] > 0


def test_exhaustive_is_lowest_t_then_lowest_primitive(oracle_built):
    """The exhaustive closest hit on a hand-made tie: two coplanar copies of one triangle, the ray hits both
    at the same t and reports primitive 0; beyond tmax or before tmin it reports a miss; the shadow query
    takes t in [0, tmax)."""
    import dataclasses
    from libyafaray_amd import scenes
    base = scenes.cornell(32, 32, spp=1)
    empty = dataclasses.replace(base, verts=np.zeros((0, 3), np.float32), tris=np.zeros((0, 3), np.int32),
                                tri_mat=np.zeros(0, np.int32), objects=[])
    tri = [(0, 0, 1), (1, 0, 1), (0, 1, 1)]
    spec = raylib.with_mesh(empty, tri + tri, [[0, 1, 2], [3, 4, 5]], "twins")
    osc = oracle_built.OracleScene(spec)
    rays = np.array([[0.25, 0.25, 0, 0, 0, 1, 0, -1],      # hits both at t = 1
                     [0.25, 0.25, 0, 0, 0, 1, 0, 1.0],     # tmax = t: excluded
                     [0.25, 0.25, 0, 0, 0, 1, 0, 1.5],
                     [0.25, 0.25, 0, 0, 0, 1, 1.0, -1],    # tmin = t: included
                     [0.25, 0.25, 0, 0, 0, 1, 1.25, -1],
                     [0.25, 0.25, 0, 0, 0, -1, 0, -1]], np.float32)
    for ex in (True, False):
        hit, prim = osc.trace_closest(rays, exhaustive=ex)
        assert prim.tolist() == [0, -1, 0, 0, -1, -1]
        assert hit[prim >= 0, 0].tolist() == [1.0, 1.0, 1.0]
        assert osc.trace_shadow(rays, exhaustive=ex).tolist() == [1, 0, 1, 1, 1, 0]
    assert osc.trace_ties(rays).tolist() == [2, 0, 2, 2, 0, 0]
