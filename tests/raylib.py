"""Ray sets with named classes, and the small scenes they are traced in, for the ray-level parity tests
(test_trace_exhaustive_cpu.py on the CPU, test_trace_queued.py and test_gpu_parity.py on the GPU).

A ray is eight float32: origin, direction, tmin, tmax (tmax < 0: unbounded) — the layout of
yafaray_amd_traceClosest.  Every class is deterministic (its own seed) and returns at most MAX_PER_CLASS
rays for a scene.

In-envelope classes (origins within 2 scene extents of the scene box's centre — the contract every
traversal must meet exactly): IN_ENVELOPE.  `far_k(spec, k)` puts the origins 10^k extents away and is
measured, not asserted, where culling is not known to be safe.  `no_ray(n)` are the closest queue's "no ray
this iteration" entries (direction x = NaN).
"""
import dataclasses

import numpy as np

from libyafaray_amd import scenes

MAX_PER_CLASS = 2048
IN_ENVELOPE = ("generic", "axis", "vertex", "edge", "grazing", "on_surface", "tmax_edge", "octants")
_SEED = {name: 1000 + 17 * k for k, name in enumerate(IN_ENVELOPE + ("no_ray", "far"))}
_TINY = np.array([0.0, -0.0, 1e-30, -1e-30], np.float32)   # below the traversals' 1e-20 direction clamp


# ---- scenes --------------------------------------------------------------------------------------------

def subset(spec, n_tris):
    """The first n_tris triangles of a scene as one object."""
    tris = spec.tris[:n_tris]
    used = np.unique(tris)
    remap = np.full(len(spec.verts), -1, np.int32)
    remap[used] = np.arange(len(used), dtype=np.int32)
    return dataclasses.replace(spec, verts=spec.verts[used], tris=remap[tris], tri_mat=spec.tri_mat[:n_tris],
                               objects=[scenes.Object("subset", 0, len(used), 0, n_tris)])


def with_mesh(spec, verts, tris, name):
    """`spec` with one more object."""
    base = len(spec.verts)
    verts = np.asarray(verts, np.float32)
    tris = np.asarray(tris, np.int32)
    return dataclasses.replace(
        spec, verts=np.concatenate([spec.verts, verts]), tris=np.concatenate([spec.tris, tris + base]),
        tri_mat=np.concatenate([spec.tri_mat, np.zeros(len(tris), np.int32)]),
        objects=list(spec.objects) + [scenes.Object(name, base, len(verts), len(spec.tris), len(tris))])


def shifted(spec, offset):
    """The whole scene (geometry, camera, lights) moved by `offset`."""
    off = np.asarray(offset, np.float32)
    sh = lambda p: tuple(float(a) + float(b) for a, b in zip(p, offset))
    cam = dataclasses.replace(spec.camera, from_=sh(spec.camera.from_), to=sh(spec.camera.to), up=sh(spec.camera.up))
    lights = [dataclasses.replace(l, from_=sh(l.from_), corner=sh(l.corner), point1=sh(l.point1), point2=sh(l.point2))
              for l in spec.lights]
    return dataclasses.replace(spec, verts=(spec.verts + off).astype(np.float32), camera=cam, lights=lights)


def sphere_slivers(offset=None):
    """cornell_sphere(n=40) (3,200 sphere triangles) plus a fan of 16 triangles 1e-4 wide across the box."""
    spec = scenes.cornell_sphere(n=40, width=32, height=32, spp=1)
    sl = []
    for k in range(16):
        x = -0.8 + 0.1 * k
        sl += [(x, -0.5, 0.2), (x + 1e-4, 0.5, 0.2), (x + 2e-4, 0.0, 1.6)]
    spec = with_mesh(spec, sl, np.arange(len(sl), dtype=np.int32).reshape(-1, 3), "slivers")
    return shifted(spec, offset) if offset is not None else spec


def dust(centre=(0.0, 0.0, 0.0), n=512, seed=5):
    """n random triangles of size about 1e-3 in a cube of side 0.05 around `centre`: around the world origin
    the builders' box pads are at their absolute floor."""
    rng = np.random.default_rng(seed)
    c = (rng.random((n, 1, 3)) - 0.5) * 0.05
    v = (c + (rng.random((n, 3, 3)) - 0.5) * 2e-3 + np.asarray(centre, np.float64)).reshape(-1, 3)
    base = scenes.cornell(32, 32, spp=1)
    empty = dataclasses.replace(base, verts=np.zeros((0, 3), np.float32), tris=np.zeros((0, 3), np.int32),
                                tri_mat=np.zeros(0, np.int32), objects=[])
    return with_mesh(empty, v, np.arange(3 * n, dtype=np.int32).reshape(-1, 3), "dust")


SCENES = {
    "cornell": lambda: scenes.cornell(32, 32, spp=1),
    "cornell-1": lambda: subset(scenes.cornell(32, 32, spp=1), 1),
    "cornell-2": lambda: subset(scenes.cornell(32, 32, spp=1), 2),
    "cornell-5": lambda: subset(scenes.cornell(32, 32, spp=1), 5),
    "sphere-slivers": lambda: sphere_slivers(),
    "sphere-slivers-shifted": lambda: sphere_slivers((1000.0, -500.0, 250.0)),
    "dust": lambda: dust(),
    "dust-333": lambda: dust((3.0, 3.0, 3.0)),
}


# ---- helpers -------------------------------------------------------------------------------------------

def scene_box(spec):
    v = spec.verts.astype(np.float64)
    lo, hi = v.min(0), v.max(0)
    return lo, hi, (lo + hi) / 2, float((hi - lo).max())


def _unit(d):
    return d / np.linalg.norm(d, axis=1, keepdims=True)


def _pack(o, d, tmin=None, tmax=None):
    n = len(o)
    tmin = np.zeros(n) if tmin is None else np.broadcast_to(tmin, (n,))
    tmax = np.full(n, -1.0) if tmax is None else np.broadcast_to(tmax, (n,))
    return np.concatenate([o, d, np.reshape(tmin, (n, 1)), np.reshape(tmax, (n, 1))], 1).astype(np.float32)


def _origins(rng, spec, n):
    """The `generic` origin distribution: within 0.8 extents of the centre."""
    _, _, c, ext = scene_box(spec)
    return c + (rng.random((n, 3)) - 0.5) * ext * 1.6


def _bound_some(rng, dist):
    """tmax per ray: a fifth of the rays stop short of their target at `dist` (misses unless something is
    nearer), a tenth are bounded beyond it, the rest are unbounded."""
    u = rng.random(len(dist))
    f = rng.random(len(dist))
    return np.where(u < 0.2, dist * (0.2 + 0.7 * f), np.where(u < 0.3, dist * (1.1 + f), -1.0))


def _tri_points(spec):
    v = spec.verts.astype(np.float64)
    return v[spec.tris[:, 0]], v[spec.tris[:, 1]], v[spec.tris[:, 2]]


def _pick_tris(rng, spec, n):
    """n random triangles with an area (a UV sphere's pole triangles have none: no plane to graze or start on)."""
    a, b, c = _tri_points(spec)
    e1, e2 = b - a, c - a
    area = np.linalg.norm(np.cross(e1, e2), axis=1)
    good = np.flatnonzero(area > 1e-9 * np.linalg.norm(e1, axis=1) * np.linalg.norm(e2, axis=1))
    return good[rng.integers(0, len(good), n)]


def _aimed(rng, spec, p, plane_tri=None):
    """Rays at the points p (n, 3), a third each: from generic origins; from a point of the plane of the
    triangle plane_tri[i] that p[i] belongs to (outside the triangle, so the ray runs in the plane); and
    along a coordinate axis from an origin that shares p's other two coordinates exactly (exact arithmetic:
    the neighbouring triangles tie)."""
    n = len(p)
    _, _, c, ext = scene_box(spec)
    o = _origins(rng, spec, n)
    mode = np.arange(n) % 3
    if plane_tri is not None:
        a, b, cc = _tri_points(spec)
        e1, e2 = (b - a)[plane_tri], (cc - a)[plane_tri]
        s = -(0.2 + rng.random((n, 1)))
        t = -(0.2 + rng.random((n, 1)))
        inpl = p + s * e1 + t * e2
        ok = np.linalg.norm(inpl - c, axis=1) <= 1.9 * ext     # (else keep the generic origin: the envelope)
        o = np.where(((mode == 1) & ok)[:, None], inpl, o)
    axis = rng.integers(0, 3, n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    h = np.float32(ext) * np.array([0.25, 0.5, 0.125])[rng.integers(0, 3, n)]
    ax_o = p.astype(np.float32).astype(np.float64)
    ax_o[np.arange(n), axis] += sign * h
    ax_d = np.zeros((n, 3))
    ax_d[np.arange(n), axis] = -sign
    o = np.where((mode == 2)[:, None], ax_o, o)
    d = p - o
    dist = np.linalg.norm(d, axis=1)
    d = np.where((mode == 2)[:, None], ax_d, d / np.maximum(dist, 1e-30)[:, None])
    return _pack(o, d, None, _bound_some(rng, dist))


# ---- classes -------------------------------------------------------------------------------------------

def generic(spec, n=MAX_PER_CLASS, seed=None):
    """The distribution of the earlier ray tests: uniform origins, normal directions, 30 % bounded."""
    rng = np.random.default_rng(_SEED["generic"] if seed is None else seed)
    _, _, c, ext = scene_box(spec)
    o = c + (rng.random((n, 3)) - 0.5) * ext * 1.6
    d = _unit(rng.normal(size=(n, 3)))
    tmax = np.where(rng.random(n) < 0.3, rng.random(n) * ext, -1.0)
    return _pack(o, d, None, tmax)


def axis(spec, n=MAX_PER_CLASS):
    """One or two direction components exactly +0, -0 or +-1e-30; half of the origins lie exactly on a
    coordinate of some vertex (on the planes of boxes)."""
    rng = np.random.default_rng(_SEED["axis"])
    _, _, c, ext = scene_box(spec)
    o = _origins(rng, spec, n).astype(np.float32)
    on = np.arange(n) % 2 == 0
    k = rng.integers(0, 3, n)
    vert = spec.verts[rng.integers(0, len(spec.verts), n)]
    o[on, k[on]] = vert[on, k[on]]
    d = _unit(rng.normal(size=(n, 3))).astype(np.float32)
    two = rng.random(n) < 0.5
    keep = rng.integers(0, 3, n)                       # two tiny components: this one stays (+-1)
    kill = rng.integers(0, 3, n)                       # one tiny component: this one goes
    for i in range(n):
        if two[i]:
            s = np.float32(1.0 if d[i, keep[i]] >= 0 else -1.0)
            d[i] = _TINY[rng.integers(0, 4, 3)]
            d[i, keep[i]] = s
        else:
            rest = [a for a in range(3) if a != kill[i]]
            nrm = np.hypot(d[i, rest[0]], d[i, rest[1]])
            d[i, rest] = d[i, rest] / nrm
            d[i, kill[i]] = _TINY[rng.integers(0, 4)]
    tmax = np.where(rng.random(n) < 0.3, rng.random(n) * ext, -1.0)
    return _pack(o, d, None, tmax)


def vertex(spec, n=MAX_PER_CLASS):
    """Aimed at mesh vertices (hits at u, v, u + v in {0, 1}; exact ties between the triangles around one)."""
    rng = np.random.default_rng(_SEED["vertex"])
    tri = rng.integers(0, len(spec.tris), n)
    corner = rng.integers(0, 3, n)
    p = spec.verts[spec.tris[tri, corner]].astype(np.float64)
    return _aimed(rng, spec, p, tri)


def edge(spec, n=MAX_PER_CLASS):
    """Aimed at points on triangle edges (shared between two triangles in every mesh here)."""
    rng = np.random.default_rng(_SEED["edge"])
    tri = rng.integers(0, len(spec.tris), n)
    e = rng.integers(0, 3, n)
    a = spec.verts[spec.tris[tri, e]].astype(np.float64)
    b = spec.verts[spec.tris[tri, (e + 1) % 3]].astype(np.float64)
    s = np.where(np.arange(n) % 2 == 0, np.array([0.5, 0.25, 0.75, 0.125])[rng.integers(0, 4, n)], rng.random(n))
    p = a + (b - a) * s[:, None]
    return _aimed(rng, spec, p, tri)


def grazing(spec, n=MAX_PER_CLASS):
    """Directions 1e-6 ... 1e-3 rad off a triangle's plane, through a point of its interior."""
    rng = np.random.default_rng(_SEED["grazing"])
    _, _, c, ext = scene_box(spec)
    a, b, cc = _tri_points(spec)
    tri = _pick_tris(rng, spec, n)
    a, e1, e2 = a[tri], (b - a)[tri], (cc - a)[tri]
    u = 0.15 + 0.5 * rng.random((n, 1))
    v = 0.15 + (0.7 - u) * rng.random((n, 1))
    p = a + u * e1 + v * e2
    nrm = _unit(np.cross(e1, e2))
    phi = rng.random((n, 1)) * 2 * np.pi
    t1 = _unit(e1)
    t2 = np.cross(nrm, t1)
    inpl = t1 * np.cos(phi) + t2 * np.sin(phi)
    ang = 10.0 ** (-6 + 3 * rng.random((n, 1))) * np.where(rng.random((n, 1)) < 0.5, -1.0, 1.0)
    d = _unit(inpl * np.cos(ang) + nrm * np.sin(ang))
    dist = (0.05 + 0.6 * rng.random(n)) * ext
    o = p - d * dist[:, None]
    return _pack(o, d, None, _bound_some(rng, dist))


def on_surface(spec, n=MAX_PER_CLASS):
    """Origins at barycentric points of triangles, as bounce and light rays have; tmin 0 or the scene's
    ray_min_dist; directions into both hemispheres and exactly tangent."""
    rng = np.random.default_rng(_SEED["on_surface"])
    _, _, c, ext = scene_box(spec)
    v = spec.verts
    tri = _pick_tris(rng, spec, n)
    a, b, cc = v[spec.tris[tri, 0]], v[spec.tris[tri, 1]], v[spec.tris[tri, 2]]
    u = rng.random((n, 1)).astype(np.float32)
    w = (rng.random((n, 1)) * (1 - u)).astype(np.float32)
    # a fifth of the points on an edge or a corner of their triangle
    snap = np.arange(n) % 5 == 0
    u[snap] = np.float32(0.0)
    w[snap & (np.arange(n) % 10 == 0)] = np.float32(0.0)
    p = (np.float32(1) - u - w) * a + u * b + w * cc          # float32, as the shading point is
    e1, e2 = (b - a).astype(np.float64), (cc - a).astype(np.float64)
    nrm = _unit(np.cross(e1, e2))
    t1 = _unit(e1)
    t2 = np.cross(nrm, t1)
    phi = rng.random((n, 1)) * 2 * np.pi
    inpl = t1 * np.cos(phi) + t2 * np.sin(phi)
    cos_t = np.sqrt(rng.random((n, 1)))
    hemi = inpl * np.sqrt(1 - cos_t ** 2) + nrm * cos_t
    kind = np.arange(n) % 3
    d = np.where((kind == 0)[:, None], hemi, np.where((kind == 1)[:, None], -hemi, inpl))
    tmin = np.where(rng.random(n) < 0.5, 0.0, spec.render.ray_min_dist)
    tmax = np.where(rng.random(n) < 0.3, rng.random(n) * ext, -1.0)
    return _pack(p, d, tmin, tmax)


def octants(spec, n=MAX_PER_CLASS):
    """All 8 direction sign combinations times 3 major axes (near / far plane selection)."""
    rng = np.random.default_rng(_SEED["octants"])
    _, _, c, ext = scene_box(spec)
    per = n // 24
    ds = []
    for sx in (-1, 1):
        for sy in (-1, 1):
            for sz in (-1, 1):
                for major in range(3):
                    m = 0.05 + 0.9 * rng.random((per, 3))
                    m[:, major] = 1.0 + rng.random(per)
                    ds.append(_unit(m * np.array([sx, sy, sz])))
    d = np.concatenate(ds)
    o = _origins(rng, spec, len(d))
    tmax = np.where(rng.random(len(d)) < 0.3, rng.random(len(d)) * ext, -1.0)
    return _pack(o, d, None, tmax)


def tmax_edge(spec, ref_closest, n=MAX_PER_CLASS):
    """Bounded rays around their own hit: tmax = the reference t, one ULP above and below it, 0; and
    unbounded ones whose tmin lies just past t.  ref_closest(rays) -> (t, prim) is the reference."""
    per = n // 5
    base = np.concatenate([generic(spec, per, seed=_SEED["tmax_edge"]), vertex(spec, per)[::3], on_surface(spec, per)[::3]])
    base[:, 6] = 0.0
    base[:, 7] = -1.0
    t, prim = ref_closest(base)
    base, t = base[prim >= 0][:per], t[prim >= 0][:per].astype(np.float32)
    out = []
    for tm in (t, np.nextafter(t, np.float32(np.inf)), np.nextafter(t, np.float32(-np.inf)), np.zeros_like(t)):
        r = base.copy()
        r[:, 7] = tm
        out.append(r)
    r = base.copy()
    r[:, 6] = np.nextafter(t, np.float32(np.inf)) * np.float32(1.001)
    out.append(r)
    return np.concatenate(out) if len(base) else np.zeros((0, 8), np.float32)


def no_ray(n, seed=None):
    """Closest-queue entries that carry no ray: direction x = NaN."""
    rng = np.random.default_rng(_SEED["no_ray"] if seed is None else seed)
    r = rng.normal(size=(n, 8)).astype(np.float32)
    r[:, 3] = np.nan
    r[:, 6] = 0.0
    r[:, 7] = -1.0
    return r


def far_k(spec, k, n=MAX_PER_CLASS):
    """Outside the envelope: origins 10^k scene extents from the centre, aimed at triangle interiors,
    vertices and points on edges."""
    rng = np.random.default_rng(_SEED["far"] + k)
    _, _, c, ext = scene_box(spec)
    a, b, cc = _tri_points(spec)
    tri = rng.integers(0, len(spec.tris), n)
    a, b, cc = a[tri], b[tri], cc[tri]
    kind = np.arange(n) % 3
    s = rng.random((n, 1))
    p = np.where((kind == 0)[:, None], (a + b + cc) / 3 + ((a + b + cc) / 3 - a) * (rng.random((n, 1)) - 0.5) * 0.5,
                 np.where((kind == 1)[:, None], a, a + (b - a) * s))
    o = c + _unit(rng.normal(size=(n, 3))) * ext * 10.0 ** k
    d = _unit(p - o)
    return _pack(o, d, None, None)


def ray_classes(spec, ref_closest):
    """{class: rays} of every in-envelope class for a scene."""
    out = {"generic": generic(spec), "axis": axis(spec), "vertex": vertex(spec), "edge": edge(spec),
           "grazing": grazing(spec), "on_surface": on_surface(spec), "tmax_edge": tmax_edge(spec, ref_closest),
           "octants": octants(spec)}
    for name, r in out.items():
        assert r.dtype == np.float32 and r.shape[1] == 8 and len(r) <= MAX_PER_CLASS, name
        assert in_envelope(spec, r), name
    return out


def in_envelope(spec, rays):
    _, _, c, ext = scene_box(spec)
    return bool((np.linalg.norm(rays[:, :3].astype(np.float64) - c, axis=1) <= 2.0 * ext).all())


def shadow_ray_of(rays):
    """Accelerator::isShadowed's preparation of a light ray, in float32 as the product does it: the origin
    moves by tmin along the direction, t_max = tmax - 2 tmin (unbounded stays unbounded), tmin = 0."""
    r = np.ascontiguousarray(rays, np.float32).copy()
    tmin = r[:, 6:7].copy()
    r[:, :3] = r[:, :3] + r[:, 3:6] * tmin
    # (a negative t_max admits no hit; 0 says the same in this layout, where a negative tmax means unbounded)
    r[:, 7] = np.where(r[:, 7] >= 0, np.maximum(r[:, 7] - np.float32(2) * tmin[:, 0], np.float32(0)), np.float32(-1.0))
    r[:, 6] = 0.0
    return r


# ---- the reference, computed once per scene and shared by the tests ---------------------------------------

_cache = {}


def scene_rays(name, oracle):
    """(spec, {class: rays}, {class: (t, prim, occluded, ties)}) of SCENES[name]: the exhaustive reference of
    every in-envelope class (oracle = the oracle.oracle module); occluded is of shadow_ray_of(rays)."""
    if name not in _cache:
        spec = SCENES[name]()
        osc = oracle.OracleScene(spec)

        def closest(r):
            hit, prim = osc.trace_closest(r, exhaustive=True)
            return hit[:, 0].copy(), prim

        rays = ray_classes(spec, closest)
        ref = {}
        for cls, r in rays.items():
            t, prim = closest(r)
            ref[cls] = (t, prim, osc.trace_shadow(shadow_ray_of(r), exhaustive=True), osc.trace_ties(r))
            for a in ref[cls]:
                a.setflags(write=False)
            r.setflags(write=False)
        _cache[name] = (spec, rays, ref)
    return _cache[name]


FAR_K = (1, 2, 3, 4)
_far_cache = {}


def far_rays(name, oracle):
    """{k: (rays, t, prim, occluded)} of SCENES[name]: far_k with its exhaustive reference."""
    if name not in _far_cache:
        spec = scene_rays(name, oracle)[0]
        osc = oracle.OracleScene(spec)
        out = {}
        for k in FAR_K:
            r = far_k(spec, k)
            hit, prim = osc.trace_closest(r, exhaustive=True)
            out[k] = (r, hit[:, 0].copy(), prim, osc.trace_shadow(shadow_ray_of(r), exhaustive=True))
            for a in out[k]:
                a.setflags(write=False)
        _far_cache[name] = out
    return _far_cache[name]
