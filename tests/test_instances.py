"""Object instances: yafaray_addInstance / yafaray_addInstanceArray, expanded on the device.

An instance is every primitive of its base under obj_to_world (the reference's ObjectInstance /
PrimitiveInstance); the library expands them per primitive into the flat arrays the renderer consumes
(instexpand.hip).  The rules (DESIGN.md "Object instances") are restated here in numpy float32, one
rounding per operation (libyafaray_amd.scenes: xform_points, xform_vectors, normalize_f32, face_normals),
and compared bit for bit; signs of zero count as equal.

Bounds: geometry and rays bit-exact (both sides evaluate the same float expressions in the same order,
every operation correctly rounded); images weights equal, values <= 4 ULP, photon counts equal — the
project's bar for images against the oracle (tests/test_gpu_parity.py).
"""
import dataclasses
import math

import numpy as np
import pytest

from libyafaray_amd import scenes

ULP_TOL = 4


def ulp_diff(a, b):
    a = np.ascontiguousarray(a, np.float32).view(np.int32).astype(np.int64)
    b = np.ascontiguousarray(b, np.float32).view(np.int32).astype(np.int64)
    a = np.where(a < 0, -(a & 0x7fffffff), a)
    b = np.where(b < 0, -(b & 0x7fffffff), b)
    return np.abs(a - b)


# ---------------------------------------------------------------------------------------------
# matrices
# ---------------------------------------------------------------------------------------------
def axis_rotation(axis, deg):
    x, y, z = np.asarray(axis, np.float64) / np.linalg.norm(axis)
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    C = 1.0 - c
    return np.array([[c + x * x * C, x * y * C - z * s, x * z * C + y * s],
                     [y * x * C + z * s, c + y * y * C, y * z * C - x * s],
                     [z * x * C - y * s, z * y * C + x * s, c + z * z * C]])


def m34(r, t=(0.0, 0.0, 0.0)):
    return np.concatenate([np.asarray(r, np.float64), np.asarray(t, np.float64).reshape(3, 1)], 1).astype(np.float32)


GENERAL = [
    m34(axis_rotation((1.0, 2.0, 3.0), 37.3), (0.31, -0.17, 0.83)),            # an irrational rotation
    m34(np.diag([1.7, 0.3, 2.9]), (-0.6, 0.45, 0.1)),                             # a non-uniform scale
    m34([[1.0, 0.37, 0.11], [0.0, 1.0, 0.53], [0.0, 0.0, 1.0]], (0.2, -0.1, 0.3)),  # a shear
    m34(axis_rotation((0.3, -1.0, 0.2), 112.0) @ np.diag([-1.1, 0.9, 0.7]), (0.05, 0.6, -0.4)),   # a mirror
    np.zeros((3, 4), np.float32),                                                   # normalize leaves zero
]
assert np.linalg.det(GENERAL[3][:, :3].astype(np.float64)) < 0


def matrices(n, seed=5, spread=2.0):
    """The five general matrices, then random rotation * non-uniform scale + translation."""
    rng = np.random.default_rng(seed)
    out = list(GENERAL[:n])
    while len(out) < n:
        r = axis_rotation(rng.normal(size=3), rng.uniform(0, 360)) @ np.diag(rng.uniform(0.2, 1.3, 3) * rng.choice([-1, 1], 3))
        out.append(m34(r, rng.uniform(-spread, spread, 3)))
    return out


# ---------------------------------------------------------------------------------------------
# scenes issued call by call (instances between the meshes), and their numpy expansion
# ---------------------------------------------------------------------------------------------
@dataclasses.dataclass
class Mesh:
    name: str
    verts: np.ndarray                  # (n, 3) float32
    tris: np.ndarray                   # (m, 3) local indices
    is_base: bool = False
    visibility: str = "normal"
    orco: bool = False
    uv: bool = False
    normals: np.ndarray = None         # exported per-vertex normals, added after the first `flat_tris` triangles
    flat_tris: int = 0                 # ... so these triangles carry -1 normal indices

    def tri_mat(self):
        return (np.arange(len(self.tris)) // 3 % 2).astype(np.int32)   # runs of three per material


def strip(n_tris, seed, scale=0.5):
    rng = np.random.default_rng(seed)
    v = (rng.uniform(-1, 1, (n_tris + 2, 3)) * scale).astype(np.float32)
    t = np.stack([np.arange(n_tris), np.arange(n_tris) + 1, np.arange(n_tris) + 2], 1).astype(np.int32)
    return v, t


def icosphere(level=2):
    """20 * 4^level triangles on the unit sphere (level 2: 320)."""
    t = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
         (-t, 0, -1), (-t, 0, 1)]
    f = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
         (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    v = [np.asarray(p, np.float64) / np.linalg.norm(p) for p in v]
    for _ in range(level):
        mid, nf = {}, []

        def m(a, b):
            k = (min(a, b), max(a, b))
            if k not in mid:
                p = v[a] + v[b]
                v.append(p / np.linalg.norm(p))
                mid[k] = len(v) - 1
            return mid[k]
        for a, b, c in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    return np.asarray(v, np.float32), np.asarray(f, np.int32)


def issue(product, items, materials=2):
    """The C API calls for `items` (Mesh objects and (base name, matrix) instances) in their order."""
    yi = product.Interface()
    yi.createScene()
    for k in range(materials):
        yi.paramsClearAll()
        yi.paramsSetString("type", "shinydiffusemat")
        yi.paramsSetColor("color", 0.2 + 0.3 * k, 0.5, 0.7, 1.0)
        yi.createMaterial("m%d" % k)
    for it in items:
        if not isinstance(it, Mesh):
            assert yi.addInstance(it[0], it[1]), yi.last_error()
            continue
        yi.paramsClearAll()
        yi.paramsSetString("type", "mesh")
        yi.paramsSetBool("has_orco", it.orco)
        yi.paramsSetBool("has_uv", it.uv)
        yi.paramsSetBool("is_base_object", it.is_base)
        yi.paramsSetString("visibility", it.visibility)
        assert yi.createObject(it.name)
        for v in it.verts:
            if it.orco:
                yi.addVertexWithOrco(*map(float, v), *map(float, v * 2 + 1))
            else:
                yi.addVertex(*map(float, v))
        if it.uv:
            for v in it.verts:
                yi.addUv(float(v[0]), float(v[1]))
        mats = it.tri_mat()
        for k, (a, b, c) in enumerate(it.tris):
            if it.normals is not None and k == it.flat_tris:
                for n in it.normals:
                    yi.addNormal(*map(float, n))
            yi.setCurrentMaterial("m%d" % mats[k])
            if it.uv:
                assert yi.addTriangleWithUv(int(a), int(b), int(c), int(a), int(b), int(c))
            else:
                assert yi.addTriangle(int(a), int(b), int(c))
        assert yi.endObject()
    return yi


def expand(items):
    """numpy restatement of the expansion: per output primitive the world vertices (n, 3, 3), the geometric
    normal, the three vertex normals (the geometric normal where the mesh has no normals) and the material."""
    meshes = {it.name: it for it in items if isinstance(it, Mesh)}
    V, NG, VN, MAT = [], [], [], []
    for it in items:
        mesh, m = (it, None) if isinstance(it, Mesh) else (meshes[it[0]], it[1])
        if mesh.visibility == "invisible" or (m is None and mesh.is_base) or not len(mesh.tris):
            continue
        ng_base = scenes.face_normals(mesh.verts, mesh.tris)
        if m is None:
            verts, ng = mesh.verts, ng_base
        else:
            verts, ng = scenes.xform_points(m, mesh.verts), scenes.normalize_f32(scenes.xform_vectors(m, ng_base))
        vn = np.repeat(ng[:, None, :], 3, 1)
        if mesh.normals is not None:
            n = mesh.normals if m is None else scenes.normalize_f32(scenes.xform_vectors(m, mesh.normals))
            vn[mesh.flat_tris:] = n[mesh.tris[mesh.flat_tris:]]
        V.append(verts[mesh.tris])
        NG.append(ng)
        VN.append(vn)
        MAT.append(mesh.tri_mat())
    return (np.concatenate(V).astype(np.float32), np.concatenate(NG).astype(np.float32), np.concatenate(VN).astype(np.float32),
            np.concatenate(MAT))


def check_primitives(yi, items):
    p = yi.primitives()
    v, ng, vn, mat = expand(items)
    assert len(p["material"]) == len(mat)
    assert np.array_equal(p["material"], mat)
    for name, got, want in (("verts", p["verts"], v), ("ng", p["ng"], ng), ("vnormals", p["vnormals"], vn)):
        bad = ~((got == want) | (np.isnan(got) & np.isnan(want)))
        assert not bad.any(), f"{name}: {bad.sum()} values differ, first at {np.argwhere(bad)[0]}: {got[bad][0]!r} vs {want[bad][0]!r}"


def mixed_scene(n_tris, n_inst):
    """A plain mesh, a flat base with n_inst instances, a visible base with exported normals (its first
    triangles without: -1 normal indices), orco and uv and its instances, a plain mesh after them."""
    bv, bt = strip(n_tris, 100 + n_tris)
    sv, st = strip(7, 3)
    rng = np.random.default_rng(9)
    sn = rng.normal(size=sv.shape).astype(np.float32)   # not unit length: normalize has work to do
    ms = matrices(n_inst, seed=n_tris)
    items = [Mesh("before", *strip(5, 1)), Mesh("base", bv, bt, is_base=True)]
    items += [("base", m) for m in ms[:(n_inst + 1) // 2]]
    items += [Mesh("shown", sv, st, orco=True, uv=True, normals=sn, flat_tris=3)]
    items += [("shown", m) for m in GENERAL] + [("base", m) for m in ms[(n_inst + 1) // 2:]]
    items += [Mesh("after", *strip(4, 2), orco=True)]
    return items


# ---------------------------------------------------------------------------------------------
# CPU
# ---------------------------------------------------------------------------------------------
def test_abi_add_instance(product):
    yi = product.Interface()
    scenes.apply(scenes.cornell_instanced(16, 12, spp=1), yi)
    first = yi.getNextFreeId()
    assert yi.addInstance("cube", GENERAL[0])
    assert yi.getNextFreeId() == first + 1
    # the reference's message (scene.cc:1013-1030); the reference itself dereferences end() first
    assert not yi.addInstance("no_such_base", GENERAL[0])
    assert "Base mesh for instance doesn't exist" in yi.last_error() and "no_such_base" in yi.last_error()
    assert yi.addInstanceArray("cube", GENERAL[0])
    assert yi.getNextFreeId() == first + 2
    # instances are named <base>-<id>: an instance of an instance is refused
    assert not yi.addInstance("cube-%d" % first, GENERAL[0])
    assert "itself an instance" in yi.last_error()
    # a base need not be a base object, nor ended
    yi.paramsClearAll()
    yi.paramsSetString("type", "mesh")
    assert yi.createObject("open")
    assert yi.addInstance("open", GENERAL[1])
    # clearAll forgets the instances with the objects
    yi.clearAll()
    yi.createScene()
    assert not yi.addInstance("cube", GENERAL[0])
    yi.close()


def _cube(spec):
    c = next(o for o in spec.objects if o.name == "cube")
    return spec.verts[c.v0:c.v0 + c.nv], spec.tris[c.t0:c.t0 + c.nt] - c.v0


def test_flatten_instances_precondition():
    """The image tests compare against the flattened scene, whose geometric normals are recomputed from
    the transformed vertices: both normal rules must agree on every face of cornell_instanced.  The same
    check fails for a 17 degree rotation (the Cornell short box's placement) and for a mirror."""
    spec = scenes.cornell_instanced()
    v, t = _cube(spec)
    assert len(spec.instances) == 3 and len(t) == 12
    for base, m in spec.instances:
        assert base == "cube" and scenes.instance_normal_rules_agree(v, t, m).all()
    rot17 = m34(axis_rotation((0, 0, 1), 17.0) * 0.6, (0.35, -0.25, 0.3))
    assert not scenes.instance_normal_rules_agree(v, t, rot17).all()
    assert not scenes.instance_normal_rules_agree(v, t, m34(np.diag([-1.0, 1.0, 1.0]))).any()
    flat = scenes.flatten_instances(spec)
    assert not flat.instances and [o.name for o in flat.objects][:5] == ["floor", "ceiling", "back", "left", "right"]
    assert len(flat.objects) == 8 and not any(o.is_base for o in flat.objects) and len(flat.tris) == 10 + 36
    for k, (_, m) in enumerate(spec.instances):
        o = flat.objects[5 + k]
        assert np.array_equal(flat.verts[o.v0:o.v0 + o.nv], scenes.xform_points(m, v))
        assert np.array_equal(flat.tris[o.t0:o.t0 + o.nt] - o.v0, t)


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_inst", [1, 3, 130])
@pytest.mark.parametrize("n_tris", [1, 63, 64, 65, 257])
def test_expanded_geometry_bitexact(product, n_tris, n_inst):
    items = mixed_scene(n_tris, n_inst)
    yi = issue(product, items)
    check_primitives(yi, items)
    yi.close()


@pytest.mark.gpu
def test_expanded_geometry_without_attributes_and_array_call(product):
    """No mesh has normals and no material has shader nodes: no attribute rows exist.  addInstanceArray
    leaves the same scene as the 16-float call."""
    bv, bt = strip(65, 4)
    a = [Mesh("base", bv, bt, is_base=True, orco=True, uv=True)] + [("base", m) for m in GENERAL] + [Mesh("after", *strip(3, 8))]
    yi = issue(product, a)
    check_primitives(yi, a)
    yj = issue(product, [a[0]])
    for _, m in a[1:6]:
        assert yj.addInstanceArray("base", m)
    p, q = yi.primitives(0, 5 * 65), yj.primitives()
    for k in p:
        assert np.array_equal(p[k].view(np.uint32), q[k].view(np.uint32)), k
    yi.close()
    yj.close()


def ray_scene(items):
    """The numpy-expanded scene as a plain SceneSpec for the oracle, and 2,048 rays aimed at the instances."""
    v, _, _, mat = expand(items)
    base = scenes.cornell(16, 16, spp=1)
    verts = v.reshape(-1, 3)
    tris = np.arange(len(verts), dtype=np.int32).reshape(-1, 3)
    spec = dataclasses.replace(base, verts=verts, tris=tris, tri_mat=mat.astype(np.int32), materials=base.materials[:2],
                               objects=[scenes.Object("all", 0, len(verts), 0, len(tris))])
    rng = np.random.default_rng(21)
    n = 2048
    fin = v[np.isfinite(v).all((1, 2)) & (np.abs(v).max((1, 2)) > 0)]
    tri = fin[rng.integers(0, len(fin), n)]
    w = rng.dirichlet((1.0, 1.0, 1.0), n)
    target = (tri * w[:, :, None]).sum(1)
    lo, hi = fin.reshape(-1, 3).min(0), fin.reshape(-1, 3).max(0)
    o = (lo + hi) / 2 + (rng.random((n, 3)) - 0.5) * (hi - lo).max() * 1.5
    d = target - o
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    tmax = np.where(rng.random((n, 1)) < 0.3, rng.random((n, 1)) * (hi - lo).max(), -1.0)
    return spec, np.concatenate([o, d, np.zeros((n, 1)), tmax], 1).astype(np.float32)


def check_rays(product, oracle_built, items):
    spec, rays = ray_scene(items)
    yi = issue(product, items)
    t, prim = yi.trace_closest(rays)
    occ = yi.trace_shadow(rays)
    n_prims = yi.L.yafaray_amd_getPrimitives(yi.h, 0, 0, None, None, None, None)
    yi.close()
    assert n_prims == len(spec.tris)
    osc = oracle_built.OracleScene(spec)
    ohit, oprim = osc.trace_closest(rays)
    assert np.array_equal(prim, oprim), f"{(prim != oprim).sum()} primitive mismatches"
    hit = oprim >= 0
    assert hit.mean() > 0.5
    assert np.array_equal(t[hit].view(np.uint32), ohit[hit, 0].view(np.uint32))
    assert np.array_equal(occ, osc.trace_shadow(rays))


@pytest.mark.gpu
@pytest.mark.parametrize("build", ["host", "gpu"])
def test_rays_small_scene_bitexact(product, oracle_built, monkeypatch, build):
    """Case a: the host's SAH builder on the vertices copied back; case b: the same scene built on the device."""
    if build == "gpu":
        monkeypatch.setenv("YAFARAY_AMD_BVH_BUILD", "gpu")
    check_rays(product, oracle_built, mixed_scene(65, 3))


@pytest.mark.gpu
def test_rays_large_scene_bitexact(product, oracle_built):
    """Case c: 300 instances of a 320-triangle sphere, 96,000 primitives: the default device build and the BVH8."""
    sv, st = icosphere(2)
    assert len(st) == 320
    items = [Mesh("ball", (sv * 0.2).astype(np.float32), st, is_base=True)] + [("ball", m) for m in matrices(300, seed=2)]
    assert 300 * 320 >= 65536
    check_rays(product, oracle_built, items)


def pm(spec, fg):
    r = dataclasses.replace(spec.render, pm_photons=20000, pm_search=50, pm_diffuse_radius=0.1, pm_bounces=5, pm_caustics=False,
                            pm_final_gather=fg, fg_samples=4)
    return dataclasses.replace(spec, render=r)


IMAGE_CASES = {
    "directlighting": lambda: scenes.cornell_instanced(80, 60, spp=4, integrator="directlighting"),
    "pathtracing": lambda: scenes.cornell_instanced(80, 60, spp=4, integrator="pathtracing", bounces=4, rr=False),
    "photonmapping": lambda: pm(scenes.cornell_instanced(80, 60, spp=4, integrator="photonmapping"), False),
    "photonmapping-fg": lambda: pm(scenes.cornell_instanced(80, 60, spp=4, integrator="photonmapping"), True),
}


def compare_image(rgba, w, orgba, ow):
    assert np.array_equal(w.view(np.uint32), ow.view(np.uint32)), "film weights differ"
    u = ulp_diff(rgba, orgba)
    assert u.max() <= ULP_TOL, f"{(u > ULP_TOL).sum()} values > {ULP_TOL} ULP, max {u.max()} at {np.unravel_index(u.argmax(), u.shape)}"


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(IMAGE_CASES))
def test_images_match_flattened_oracle(product, oracle_built, case):
    spec = IMAGE_CASES[case]()
    rgba, w, st = product.render_spec(spec)
    o = oracle_built.OracleScene(scenes.flatten_instances(spec), threads=8)
    orgba, ow, _ = o.render()
    if case.startswith("photonmapping"):
        dpos, *_ = o.photon_map("diffuse")
        assert st["photons"] == len(dpos)
    compare_image(rgba, w, orgba, ow)
    assert rgba[..., :3].max() > 0.1


@pytest.mark.gpu
def test_two_members_equal_one(product):
    spec = scenes.cornell_instanced(80, 60, spp=2, integrator="pathtracing", bounces=3)
    a, wa, _ = product.render_spec(spec)
    b, wb, st = product.render_spec(spec, members=2)
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32)) and np.array_equal(wa, wb)


@pytest.mark.gpu
def test_instance_added_after_a_render(product):
    spec = scenes.cornell_instanced(64, 48, spp=1, integrator="directlighting")
    late = dataclasses.replace(spec, instances=spec.instances[:2])
    yi = product.Interface()
    scenes.apply(late, yi)
    yi.render()
    first, _ = yi.film()
    first = first.copy()
    assert yi.addInstance(*spec.instances[2])
    yi.render()
    again, wa = yi.film()
    yi.close()
    fresh, wf, _ = product.render_spec(spec)
    assert np.array_equal(again.view(np.uint32), fresh.view(np.uint32)) and np.array_equal(wa, wf)
    assert not np.array_equal(first, again)


@pytest.mark.gpu
def test_meshlight_on_an_instance_fails_loudly(product):
    spec = scenes.cornell_instanced(32, 24, spp=1, integrator="directlighting")
    name = "cube-%d" % (len(spec.objects) + 1)   # the first instance (scenes.apply adds them after the objects)
    lamp = scenes.Light("lamp", type="meshlight", color=(1.0, 0.9, 0.75), power=3.0, object_name=name, samples=1)
    with pytest.raises(RuntimeError, match="is an instance"):
        product.render_spec(dataclasses.replace(spec, lights=[lamp]))


@pytest.mark.gpu
def test_invisible_base_hides_its_instances(product):
    bv, bt = strip(9, 6)
    hidden = [Mesh("plain", *strip(5, 1)), Mesh("base", bv, bt, visibility="invisible"), ("base", GENERAL[0]), ("base", GENERAL[1])]
    yi = issue(product, hidden)
    check_primitives(yi, hidden)
    assert len(yi.primitives()["material"]) == 5
    yi.close()


@pytest.mark.gpu
def test_expansion_beyond_int_indices_is_refused(product):
    """65,522 triangles x 11,000 instances = 720.7 M primitives: three indices per primitive no longer fit
    the int the device arrays are indexed with (2^31 / 3 = 715.8 M).  The build fails before anything is
    allocated."""
    sv, st = scenes.uv_sphere(181, center=(0, 0, 0), r=0.5)
    assert len(st) == 65522 and 3 * len(st) * 11000 > 2 ** 31 - 1
    yi = product.Interface()
    yi.createScene()
    yi.paramsClearAll()
    yi.paramsSetString("type", "shinydiffusemat")
    yi.createMaterial("m")
    yi.paramsClearAll()
    yi.paramsSetString("type", "mesh")
    yi.paramsSetBool("is_base_object", True)
    assert yi.createObject("ball")
    yi.addVertices(sv)
    yi.setCurrentMaterial("m")
    yi.addTriangles(st)
    assert yi.endObject()
    for _ in range(11000):
        assert yi.addInstance("ball", GENERAL[0])
    assert not yi.L.yafaray_amd_buildAccelerator(yi.h)
    assert "cannot index" in yi.last_error()
    yi.close()
