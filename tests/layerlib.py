"""Helpers of tests/test_layers.py: expected render-layer values that do not come from the product.

* The perspective camera at pixel centres restated in numpy float32, one rounding per operation, in the
  expression order of the reference's camera.cc:51-71, camera_perspective.cc:28-69 + 128-146 and
  plane.h:37-40 (the style of scenes.xform_points / normalize_f32).  Its rays go through
  OracleScene.trace_closest — not the product's ray seam — for t, primitive and barycentrics.
* Per-primitive values (normals, UVs, indices) evaluated from the scene spec in numpy.
* Emissive twins: a scene whose oracle *combined* render shows a per-primitive value as emission, so the
  film arithmetic of a layer can be compared with the oracle's film.
"""
import dataclasses

import numpy as np

from libyafaray_amd import scenes

F = np.float32

ALL_LAYERS = ["z-depth-abs", "z-depth-norm", "mist", "debug-normal-geom", "debug-normal-smooth", "debug-uv",
              "debug-barycentric-uvw", "adv-diffuse-color", "obj-index-abs", "obj-index-norm", "mat-index-abs",
              "mat-index-norm"]
# the reference's LayerDef::Type order of the layers above ("combined" first)
TYPE_ORDER = ["combined", "debug-barycentric-uvw", "adv-diffuse-color", "mat-index-abs", "mat-index-norm", "mist",
              "debug-normal-geom", "debug-normal-smooth", "obj-index-abs", "obj-index-norm", "debug-uv", "z-depth-abs",
              "z-depth-norm"]


def layer(type_, exported="ColorAlpha", image_type=None, name=None):
    return {"type": type_, "image_type": image_type, "exported_image_type": exported,
            "exported_image_name": name if name is not None else type_.upper()}


def _v(x):
    return np.asarray(x, F)


def _cross(a, b):
    return np.stack([a[..., 1] * b[..., 2] - a[..., 2] * b[..., 1], a[..., 2] * b[..., 0] - a[..., 0] * b[..., 2],
                     a[..., 0] * b[..., 1] - a[..., 1] * b[..., 0]], -1).astype(F)


def _dot(a, b):
    return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1] + a[..., 2] * b[..., 2]).astype(F)


def _nrm(v):
    return scenes.normalize_f32(v).reshape(np.shape(v))


def camera_frame(cam):
    """camera.cc:51-71 + camera_perspective.cc:28-69 in float32."""
    pos, look, up = _v(cam.from_), _v(cam.to), _v(cam.up)
    aspect = F(cam.aspect_ratio) * F(cam.resy) / F(cam.resx)
    cam_y, cam_z = up - pos, look - pos
    cam_x = _cross(cam_z, cam_y)
    cam_y = _cross(cam_z, cam_x)
    cam_x, cam_y, cam_z = _nrm(cam_x), _nrm(cam_y), _nrm(cam_z)
    vright, vup = cam_x, cam_y * aspect
    vto = cam_z * F(cam.focal) - (vup + vright) * F(0.5)
    vup = vup / F(cam.resy)
    vright = vright / F(cam.resx)
    near_p, far_p = pos + cam_z * F(cam.near_clip), pos + cam_z * F(cam.far_clip)
    return dict(pos=pos, vright=vright, vup=vup, vto=vto, cam_z=cam_z, near_p=near_p, far_p=far_p)


def shoot(cam, px, py):
    """PerspectiveCamera::shootRay without a lens: rays (n, 8) = from, dir, tmin, tmax."""
    assert cam.aperture == 0.0
    f = camera_frame(cam)
    px, py = _v(px).reshape(-1, 1), _v(py).reshape(-1, 1)
    d = _nrm((f["vright"][None] * px + f["vup"][None] * py + f["vto"][None]).astype(F))
    den = _dot(d, f["cam_z"][None])
    with np.errstate(divide="ignore", invalid="ignore"):
        tmin = _dot(f["cam_z"], f["near_p"] - f["pos"]) / den
        tmax = _dot(f["cam_z"], f["far_p"] - f["pos"]) / den
    n = len(d)
    return np.concatenate([np.broadcast_to(f["pos"], (n, 3)), d, tmin.reshape(n, 1), tmax.reshape(n, 1)], 1).astype(F)


def pixel_centre_rays(spec):
    """The 1-spp camera rays of every film pixel, row-major (integrator_tiled.cc:313-342: dx = dy = 0.5,
    camera pixel = film pixel + crop origin)."""
    r = spec.render
    y, x = np.mgrid[0:r.height, 0:r.width]
    return shoot(spec.camera, (x + r.xstart).astype(F).reshape(-1) + F(0.5), (y + r.ystart).astype(F).reshape(-1) + F(0.5))


def first_hits(oracle, spec):
    """Oracle closest hits of the pixel-centre rays: t (the camera's tmax on a miss), prim (-1), barycentrics, tmax."""
    rays = pixel_centre_rays(spec)
    hit, prim = oracle.OracleScene(spec).trace_closest(rays)
    t = np.where(prim >= 0, hit[:, 0], rays[:, 7]).astype(F)
    return dict(t=t, prim=prim, bary=hit[:, 1:4].astype(F), tmax=rays[:, 7])


def depth_range(oracle, spec):
    """TiledIntegrator::precalcDepths (integrator_tiled.cc:69-95): (min_depth_, max_depth_) as the layers use them."""
    cam = spec.camera
    if cam.far_clip > -1:
        mn, mx = F(cam.near_clip), F(cam.far_clip)
    else:
        i, j = np.mgrid[0:cam.resy, 0:cam.resx]   # shootRay(i, j): the row index as x, the column index as y
        rays = shoot(cam, i.reshape(-1).astype(F), j.reshape(-1).astype(F))
        hit, prim = oracle.OracleScene(spec).trace_closest(rays)
        tm = np.where(prim >= 0, hit[:, 0], rays[:, 7]).astype(F)
        mx = F(max(F(0.0), tm[tm > 0].max() if (tm > 0).any() else F(0.0)))
        mn = F(min(F(1e38), tm[tm >= 0].min() if (tm >= 0).any() else F(1e38)))
    if mx > 0:
        mx = F(1.0) / (mx - mn)
    return F(mn), F(mx)


def prim_object_index(spec):
    """object_index per primitive of a scene without instances (flatten_instances first)."""
    out = np.zeros(len(spec.tris), np.int64)
    for o in spec.objects:
        out[o.t0:o.t0 + o.nt] = o.object_index
    return out


def prim_material_index(spec):
    idx = np.asarray([m.mat_pass_index if m.type == "shinydiffusemat" else 0 for m in spec.materials], np.int64)
    return idx[np.asarray(spec.tri_mat)]


def highest(values):
    return max(1, int(max(values, default=0)))


def expected_layers(oracle, spec, hits=None):
    """Every in-scope layer's per-sample RGBA of the 1-spp pixel-centre render, (H, W, 4) float32 each, evaluated in
    numpy from the oracle's first hits and the spec (generateCommonLayers + integrator_tiled.cc:383-400)."""
    r = spec.render
    h = hits or first_hits(oracle, spec)
    n = r.width * r.height
    hit = h["prim"] >= 0
    p = np.where(hit, h["prim"], 0)
    t, b = h["t"], h["bary"]
    out = {}

    def put(name, rgb, alpha=None):
        v = np.zeros((n, 4), F)
        v[:, :3] = rgb
        v[:, 3] = F(1.0) if alpha is None else alpha
        v[~hit] = (0.0, 0.0, 0.0, 1.0)   # LayerDef's default colour
        out[name] = v.reshape(r.height, r.width, 4)

    def gray(name, g):
        g = g.astype(F)
        v = np.stack([g, g, g, np.where(g > 1, F(1.0), g)], -1).astype(F)   # Rgba{float}: alpha = g, then clamped to 1
        v[t < 0] = 0.0                                                       # background: fully transparent
        out[name] = v.reshape(r.height, r.width, 4)

    mn, mx = depth_range(oracle, spec)
    gray("z-depth-abs", t)
    gray("z-depth-norm", F(1.0) - (t - mn) * mx)
    gray("mist", (t - mn) * mx)
    verts, tris = np.asarray(spec.verts, F), np.asarray(spec.tris)
    ng = scenes.face_normals(verts, tris)
    put("debug-normal-geom", (ng[p] + F(1.0)) * F(0.5))
    if spec.normals is not None:
        vn = np.asarray(spec.normals, F)[tris[p]]   # (n, 3 vertices, 3)
        sn = _nrm((b[:, 0:1] * vn[:, 0] + b[:, 1:2] * vn[:, 1] + b[:, 2:3] * vn[:, 2]).astype(F))
    else:
        sn = ng[p]
    put("debug-normal-smooth", (sn + F(1.0)) * F(0.5))
    uv = b[:, :2].copy()
    if spec.uvs is not None and spec.tri_uv is not None:
        tu = np.asarray(spec.tri_uv)[p]
        has = (tu >= 0).all(1)
        w = np.asarray(spec.uvs, F)[np.where(tu >= 0, tu, 0)]   # (n, 3, 2)
        du1, du2, dv1, dv2 = (w[:, 1, 0] - w[:, 0, 0], w[:, 2, 0] - w[:, 0, 0], w[:, 1, 1] - w[:, 0, 1], w[:, 2, 1] - w[:, 0, 1])
        has &= np.abs(du1 * dv2 - dv1 * du2) > F(1e-30)      # else the implicit mapping (primitive_triangle.cc:141-158)
        # (objects without uv values of their own keep the implicit mapping too)
        obj_uv = np.zeros(len(tris), bool)
        for o in spec.objects:
            obj_uv[o.t0:o.t0 + o.nt] = o.nuv > 0
        has &= obj_uv[p]
        m = (b[:, 0:1] * w[:, 0] + b[:, 1:2] * w[:, 1] + b[:, 2:3] * w[:, 2]).astype(F)
        uv = np.where(has[:, None], m, uv)
    put("debug-uv", np.concatenate([uv, np.zeros((n, 1), F)], 1))
    put("debug-barycentric-uvw", b)
    oi, mi = prim_object_index(spec), prim_material_index(spec)
    oh = highest(o.object_index for o in spec.objects)
    mh = highest(m.mat_pass_index for m in spec.materials if m.type == "shinydiffusemat")
    put("obj-index-abs", oi[p].astype(F)[:, None])
    put("obj-index-norm", (oi[p].astype(F) / F(oh))[:, None])
    put("mat-index-abs", mi[p].astype(F)[:, None])
    put("mat-index-norm", (mi[p].astype(F) / F(mh))[:, None])
    dc = np.asarray([[F(m.diffuse_reflect) * F(c) for c in m.color] if m.type == "shinydiffusemat" else [0, 0, 0]
                     for m in spec.materials], F)
    put("adv-diffuse-color", dc[np.asarray(spec.tri_mat)[p]])
    return out


def emissive_twin(spec, prim_rgb):
    """`spec` (no instances) with every primitive's material replaced by a double-sided light_mat emitting prim_rgb[p]
    (one material per distinct colour), no lights, direct lighting: its combined render shows the colour of the
    primitive each camera sample hits, through the film."""
    prim_rgb = np.asarray(prim_rgb, F).reshape(len(spec.tris), -1)
    if prim_rgb.shape[1] == 1:
        prim_rgb = np.repeat(prim_rgb, 3, 1)
    cols, inv = np.unique(prim_rgb, axis=0, return_inverse=True)
    mats = [scenes.Material("e%d" % k, type="light_mat", color=tuple(float(x) for x in c), power=1.0, double_sided=True)
            for k, c in enumerate(cols)]
    return dataclasses.replace(spec, materials=mats, tri_mat=np.asarray(inv, np.int32).reshape(-1), lights=[], layers=[],
                               textures=[], images=[], render=dataclasses.replace(spec.render, integrator="directlighting"))


def ulp(a, b):
    """Per-element distance in float32 steps (ordered-integer view; -0 == +0)."""
    def key(x):
        i = np.ascontiguousarray(x, F).view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7fffffff), i)
    return np.abs(key(a) - key(b))


def icosphere(level=2, center=(0.0, 0.0, 1.0), r=0.5):
    """Vertices (float32), faces, and unit vertex normals of a subdivided icosahedron."""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = [(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g), (g, 0, -1), (g, 0, 1),
         (-g, 0, -1), (-g, 0, 1)]
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
        for (a, b, c) in f:
            ab, bc, ca = m(a, b), m(b, c), m(c, a)
            nf += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        f = nf
    n = np.asarray(v, np.float64)
    return (n * r + np.asarray(center)).astype(F), np.asarray(f, np.int32), scenes.normalize_f32(n.astype(F))


def layers_scene(width=37, height=29, spp=1, tile=16, focal=1.0, **kw):
    """The Cornell box (from outside: a frame of pixels misses it) with a level-2 icosphere carrying exported vertex
    normals + smoothMesh, a UV-mapped quad, distinct object and material indices.  Every object carries vertex
    normals (apply() exports them per object): the walls' and boxes' are their vertices' directions from the room's
    centre, so debug-normal-smooth differs from debug-normal-geom everywhere."""
    s = scenes.cornell(width, height, spp=spp, bounces=2, integrator="directlighting", tile_size=tile, **kw)
    sv, st, sn = icosphere(2, center=(0.4, -0.45, 1.0), r=0.3)
    qv = np.asarray([(-0.9, -0.6, 0.05), (-0.2, -0.6, 0.05), (-0.2, -0.1, 0.6), (-0.9, -0.1, 0.6)], F)
    qt = np.asarray([(0, 1, 2), (0, 2, 3)], np.int32)
    quv = np.asarray([(0.1, 0.2), (1.7, 0.25), (1.6, 2.5), (-0.3, 2.25)], F)
    v0, t0 = len(s.verts), len(s.tris)
    verts = np.concatenate([s.verts, sv, qv])
    tris = np.concatenate([s.tris, st + v0, qt + v0 + len(sv)])
    mats = [dataclasses.replace(m, mat_pass_index=k, diffuse_reflect=d) for m, k, d in zip(s.materials, (3, 0, 7), (0.8, 1.0, 0.5))]
    mats.append(scenes.Material("blue", color=(0.2, 0.3, 0.9), diffuse_reflect=0.9, mat_pass_index=5))
    tri_mat = np.concatenate([s.tri_mat, np.full(len(st), 3, np.int32), np.full(len(qt), 1, np.int32)])
    objs = [dataclasses.replace(o, object_index=k) for o, k in zip(s.objects, (0, 2, 9, 4, 4, 1, 6))]
    objs.append(scenes.Object("ico", v0, len(sv), t0, len(st), smooth_angle=180.0, object_index=11))
    objs.append(scenes.Object("uvquad", v0 + len(sv), len(qv), t0 + len(st), len(qt), uv0=0, nuv=len(quv), object_index=3))
    room_n = scenes.normalize_f32(np.asarray(s.verts, F) - _v((0.0, 0.0, 1.0)) + _v((0.03, 0.02, 0.01)))
    quad_n = scenes.normalize_f32(_v([(0.1, -1.0, 1.0), (-0.1, -1.0, 0.9), (0.0, -0.8, 1.0), (0.2, -1.0, 1.2)]))
    tri_uv = np.full((len(tris), 3), -1, np.int32)
    tri_uv[t0 + len(st):] = qt
    cam = dataclasses.replace(s.camera, focal=focal)
    return dataclasses.replace(s, verts=verts, tris=tris, tri_mat=tri_mat, materials=mats, objects=objs, camera=cam,
                               normals=np.concatenate([room_n, sn, quad_n]).astype(F), uvs=quv, tri_uv=tri_uv)
