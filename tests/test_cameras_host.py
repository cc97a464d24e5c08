"""The architect, orthographic, equirectangular and angular cameras at the C API, the recorded reference pixels
they are tested against (tests/golden/cameras.npz, made by tests/golden/make_golden_cameras.py from the reference
library), and the cameras' numerics built for the host (tests/camera_host.cc: devmath.h's asin / atan beside the
host's libm, and properties of camera.h's ray functions).  No GPU needed."""
import ctypes as C
import json
import os
import subprocess
import tempfile

import numpy as np
import pytest

import cameralib as CL
from libyafaray_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
F = np.float32

# ---- creation and staging ----
DEFAULTS = [("architect", {}), ("orthographic", {}), ("equirectangular", {}), ("angular", {})]
COMMON = {"from": ("v", (0.1, -0.6, 1.1)), "to": ("v", (0.2, 0.4, 1.0)), "up": ("v", (0.1, -0.6, 2.1)), "resx": ("i", 48), "resy": ("i", 36),
          "aspect_ratio": ("f", 1.1), "nearClip": ("f", 0.2), "farClip": ("f", 7.5), "view_name": ("s", "")}
FULL = [
    ("architect", dict(COMMON, focal=("f", 1.4), aperture=("f", 0.1), dof_distance=("f", 3.9), bokeh_type=("s", "hexagon"),
                       bokeh_bias=("s", "edge"), bokeh_rotation=("f", 15.0))),
    ("orthographic", dict(COMMON, scale=("f", 2.9))),
    ("equirectangular", dict(COMMON)),
] + [("angular", dict(COMMON, angle=("f", 75.0), max_angle=("f", 60.0), circular=("b", c), mirrored=("b", not c), projection=("s", p)))
     for p, c in zip(CL.PROJECTIONS + ("nonsense",), (True, False, True, False, True, False))]


def _create(product, ctype, params):
    yi = product.Interface()
    yi.createScene()
    yi.paramsClearAll()
    yi.paramsSetString("type", ctype)
    for k, tv in params.items():
        scenes.set_typed(yi, k, tv)
    ok = yi.createCamera("cam")
    err = yi.last_error()
    yi.close()
    return ok, err


@pytest.mark.parametrize("ctype,params", DEFAULTS + FULL, ids=lambda v: v if isinstance(v, str) else str(len(v)) + str(v.get("projection", ("", ""))[1]))
def test_create_camera_accepts_the_four_types(product, ctype, params):
    ok, err = _create(product, ctype, params)
    assert ok == 1, err
    assert "not supported" not in err


@pytest.mark.parametrize("ctype", ["fisheye", "", "Perspective"])
def test_create_camera_still_refuses_an_unknown_type(product, ctype):
    ok, err = _create(product, ctype, {})
    assert ok == 0
    assert "not supported by the GPU core" in err


@pytest.mark.parametrize("name", CL.names())
def test_recorded_specs_stage(product, name):
    spec = CL.spec(name)
    yi = product.Interface()
    scenes.apply(spec, yi)
    err = yi.last_error()
    w, h = yi.getSceneFilmWidth(), yi.getSceneFilmHeight()
    yi.close()
    assert err == ""
    assert (w, h) == (spec.render.width, spec.render.height) == (spec.camera.resx, spec.camera.resy)
    assert (w, h) == ((CL.EQUI_W, CL.EQUI_H) if spec.camera.type == "equirectangular" else (CL.W, CL.H))


class _Rec:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*a):
            self.calls.append((name,) + tuple(x if not isinstance(x, np.ndarray) else x.tobytes() for x in a))
            return 1
        return call


def _camera_calls(spec):
    r = _Rec()
    scenes.apply(spec, r)
    end = [c[0] for c in r.calls].index("createCamera")
    start = max(i for i, c in enumerate(r.calls[:end]) if c[0] == "paramsClearAll")
    return r.calls[start + 1:end + 1]


def test_perspective_spec_issues_the_calls_it_issued():
    """The call sequence of a perspective camera, with and without depth of field, is the one before the `type`
    field existed: bench.py and every older test go through it."""
    cam = scenes.cornell(16, 12).camera
    head = [("paramsSetString", "type", "perspective"), ("paramsSetVector", "from") + cam.from_, ("paramsSetVector", "to") + cam.to,
            ("paramsSetVector", "up") + cam.up, ("paramsSetInt", "resx", 16), ("paramsSetInt", "resy", 12), ("paramsSetFloat", "focal", 1.4),
            ("paramsSetFloat", "aspect_ratio", 1.0), ("paramsSetFloat", "nearClip", 0.0), ("paramsSetFloat", "farClip", -1.0)]
    assert _camera_calls(scenes.cornell(16, 12)) == head + [("createCamera", "cam")]
    dof = scenes.cornell(16, 12).with_camera(aperture=0.1, dof_distance=3.0, bokeh_type="ring")
    assert _camera_calls(dof) == head + [("paramsSetFloat", "aperture", 0.1), ("paramsSetFloat", "dof_distance", 3.0),
                                         ("paramsSetString", "bokeh_type", "ring"), ("paramsSetString", "bokeh_bias", "uniform"),
                                         ("paramsSetFloat", "bokeh_rotation", 0.0), ("createCamera", "cam")]


def test_other_cameras_issue_their_own_parameters():
    keys = lambda name: [c[1] for c in _camera_calls(CL.spec(name)) if c[0].startswith("paramsSet")]
    assert "scale" in keys("ortho_dl") and "focal" not in keys("ortho_dl")
    # the type's own far plane (-1.0e38) unless the spec sets one
    assert "farClip" not in keys("equi_dl") and "farClip" in keys("equi_layers") and "farClip" in keys("ortho_dl")
    k = keys("ang_max_dl")
    assert {"angle", "max_angle", "circular", "mirrored", "projection"} <= set(k)
    assert "max_angle" not in keys("ang_equidistant_dl")
    with pytest.raises(ValueError):
        scenes.apply(scenes.cornell(16, 12).with_camera(type="fisheye"), _Rec())


# ---- the fixture ----
def test_fixture_matches_the_specs():
    fx = CL.fixture()
    params = json.loads(bytes(fx["params_json"]).decode())
    assert sorted(params) == sorted(CL.names())
    for name in CL.names():
        spec = CL.spec(name)
        assert params[name] == {"integrator": spec.render.integrator, "camera": CL.camera_params(spec)}, name
        a = fx[name]
        assert a.shape == (spec.render.height, spec.render.width, 4) and a.dtype == np.float32, name
        assert np.isfinite(a).all() and a[..., :3].max() > 0, name
        for layer in CL.layer_names(name):
            b = fx[name + "/" + layer]
            assert b.shape == a.shape and np.isfinite(b).all(), (name, layer)
    recorded = {k for k in fx if k != "params_json"}
    assert recorded == set(CL.names()) | {n + "/" + l for n in CL.names() for l in CL.layer_names(n)}


def test_fixture_circular_scenes_hold_the_black_surround():
    fx = CL.fixture()
    assert len(CL.circular_names()) >= 10
    for name in CL.circular_names():
        a = fx[name]
        c = CL.corners(a)
        assert (c[:, :3] == 0).all() and (np.abs(c[:, 3] - 1) < 1e-6).all(), name
        assert (a == F([0, 0, 0, 1])).all(-1).sum() > 0, name
        assert ((a[..., 3] < 1) | (a[..., :3].sum(-1) > 0)).sum() > 0, name
    # a miss of the transparent background differs from the surround
    wide = fx["ang_wide_bg_dl"]
    assert (wide[..., 3] == 0).sum() > 100 and (CL.corners(wide)[:, 3] == 1).all()
    # the square angular camera has no surround
    assert CL.corners(fx["ang_square_dl"])[:, :3].sum() > 0


# ---- the numerics, built for the host ----
@pytest.fixture(scope="module")
def ch():
    out = os.path.join(tempfile.gettempdir(), "yaf_camera_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out, os.path.join(HERE, "camera_host.cc")],
                   check=True)
    lib = C.CDLL(out)
    fp = C.POINTER(C.c_float)
    lib.ch_angular.argtypes = [fp, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_int, C.c_int, fp, C.c_int, fp, C.POINTER(C.c_int)]
    return lib


def P(a, t=C.c_float):
    return a.ctypes.data_as(C.POINTER(t))


def _inputs():
    rng = np.random.default_rng(20261021)
    n = 1 << 20
    uni = rng.uniform(-1.0, 1.0, n).astype(F)
    scaled = (rng.uniform(-1.0, 1.0, n) * np.exp2(rng.integers(-40, 3, n))).astype(F)
    raw = rng.integers(0, 1 << 32, n, dtype=np.uint64).astype(np.uint32).view(F)
    one = F(1.0)
    edges = [F(0.0), F(-0.0), one, -one, np.nextafter(one, F(0)), np.nextafter(one, F(2)), -np.nextafter(one, F(0)), -np.nextafter(one, F(2)),
             F(0.5), np.nextafter(F(0.5), F(0)), np.nextafter(F(0.5), one), F(0.975), F(np.inf), F(-np.inf), F(np.nan)]
    near_one = (one - rng.uniform(0, 1, 1 << 16) * np.exp2(rng.integers(-24, -1, 1 << 16))).astype(F)
    return np.concatenate([uni, scaled, raw, np.array(edges, F), near_one, -near_one])


@pytest.mark.parametrize("which,name", [(0, "asinf"), (1, "atanf"), (2, "math::asin")])
def test_libm_restatements_equal_the_host_libm(ch, which, name):
    """devmath.h libmAsinf / libmAtanf (and math::asin's clamp) against the host's libm, bit for bit, NaN for
    NaN, on a few million inputs: uniform in [-1, 1], random exponents, raw bit patterns, the clamp's edges."""
    x = np.ascontiguousarray(_inputs())
    dev, ref = np.empty_like(x), np.empty_like(x)
    ch.ch_libm(which, P(x), len(x), P(dev), P(ref))
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(dev), nan), name
    assert np.array_equal(dev[~nan].view(np.uint32), ref[~nan].view(np.uint32)), name
    if which == 2:
        assert not np.isnan(dev[~np.isnan(x)]).any()


def _frame():
    """An orthonormal camera frame off the axes (vright, vup, vto), float32."""
    z = np.array([0.05, 1.0, -0.06]); z /= np.linalg.norm(z)
    x = np.cross(z, [0.0, 0.0, 1.0]); x /= np.linalg.norm(x)
    y = np.cross(x, z)
    return np.ascontiguousarray(np.stack([x, y, z]).astype(F))


def _grid(w, h, step=0.25):
    xs, ys = np.meshgrid(np.arange(0, w + step, step), np.arange(0, h + step, step))
    return np.ascontiguousarray(np.stack([xs.ravel(), ys.ravel()], -1).astype(F))


def test_orthographic_rays_are_parallel_from_one_plane(ch):
    fr = _frame()
    scale, w, h = F(2.9), 48, 36
    fr_o = fr.copy()
    fr_o[0] *= scale / F(w)
    fr_o[1] *= F(0.75) * scale / F(h)
    pos = np.array([0.03, -3.9, 1.02], F)
    pxy = _grid(w, h)
    out = np.empty((len(pxy), 6), F)
    ch.ch_ortho(P(fr_o), P(pos), P(pxy), len(pxy), P(out))
    assert (out[:, 3:] == fr[2]).all()                       # vto as it stands, not normalised again
    off = (out[:, :3].astype(np.float64) - pos) @ fr[2].astype(np.float64)
    assert np.abs(off).max() < 1e-5                          # the origins lie in the plane through pos_ normal to cam_z
    span = out[:, :3].max(0) - out[:, :3].min(0)
    assert np.linalg.norm(span) > 2.9                        # and spread over scale x scale * aspect


def test_equirectangular_rays_wrap_and_level(ch):
    fr = _frame()
    w, h = 48, 24
    ys = np.arange(0, h + 0.5, 0.5, dtype=F)
    left = np.ascontiguousarray(np.stack([np.zeros_like(ys), ys], -1))
    right = np.ascontiguousarray(np.stack([np.full_like(ys, w), ys], -1))
    a, b = np.empty((len(ys), 3), F), np.empty((len(ys), 3), F)
    ch.ch_equirect(P(fr), w, h, P(left), len(ys), P(a))
    ch.ch_equirect(P(fr), w, h, P(right), len(ys), P(b))
    # u = -1 and u = +1 are the same meridian (behind the camera) up to the rounding of sin(+-pi)
    assert np.abs(a - b).max() < 1e-5
    assert (a @ fr[2] < 1e-5).all()
    xs = np.arange(0, w + 0.5, 0.5, dtype=F)
    mid = np.ascontiguousarray(np.stack([xs, np.full_like(xs, h / 2)], -1))
    c = np.empty((len(xs), 3), F)
    ch.ch_equirect(P(fr), w, h, P(mid), len(xs), P(c))
    assert np.abs(c.astype(np.float64) @ fr[1].astype(np.float64)).max() < 1e-6   # v = 0: perpendicular to vup
    centre = np.array([[w / 2, h / 2]], F)
    d = np.empty((1, 3), F)
    ch.ch_equirect(P(fr), w, h, P(centre), 1, P(d))
    assert np.abs(d[0] - fr[2]).max() < 1e-6


@pytest.mark.parametrize("projection", range(5))
def test_angular_centre_and_circle(ch, projection):
    fr = _frame()
    w, h = 48, 36
    aspect = F(0.75)
    angle = F(np.pi / 3) if projection == 4 else F(np.pi / 2)
    focal = {0: F(1) / angle, 1: F(1) / F(np.sin(angle)), 2: F(0.5) / F(np.tan(angle / 2)), 3: F(0.5) / F(np.sin(angle / 2)),
             4: F(1) / F(np.tan(angle))}[projection]

    def shoot(pxy, max_radius=F(1.0), circular=1):
        pxy = np.ascontiguousarray(np.asarray(pxy, F).reshape(-1, 2))
        out, valid = np.empty((len(pxy), 3), F), np.empty(len(pxy), np.int32)
        ch.ch_angular(P(fr), w, h, aspect, focal, max_radius, circular, projection, P(pxy), len(pxy), P(out), P(valid, C.c_int))
        return out, valid
    # the exact centre is vto (theta = 0, phi = 0)
    d, ok = shoot([w / 2, h / 2])
    assert ok[0] == 1 and np.array_equal(d[0], fr[2])
    # on the horizontal axis the radius is |u| = |1 - 2 px / resx| exactly: px = 0 has radius 1
    d, ok = shoot([[0.0, h / 2], [w, h / 2]], max_radius=F(1.0))
    assert list(ok) == [1, 1]                                  # radius == max_radius is valid
    d, ok = shoot([[0.0, h / 2], [w, h / 2]], max_radius=np.nextafter(F(1.0), F(0)))
    assert list(ok) == [0, 0]                                  # radius > max_radius is not
    d, ok = shoot([[0.0, h / 2]], max_radius=F(0.5), circular=0)
    assert ok[0] == 1                                          # nor is anything when the camera is not circular
    # at radius 1 the ray is `angle` away from vto
    d, ok = shoot([[0.0, h / 2]])
    cosang = float(d[0].astype(np.float64) @ fr[2].astype(np.float64)) / float(np.linalg.norm(d[0].astype(np.float64)))
    assert abs(np.degrees(np.arccos(np.clip(cosang, -1, 1))) - np.degrees(float(angle))) < 1.0
    # the corners lie outside the circle, the whole grid inside is valid and finite
    grid = _grid(w, h, 0.5)
    d, ok = shoot(grid)
    u = 1 - 2 * grid[:, 0] / w
    v = (2 * grid[:, 1] / h - 1) * 0.75
    r = np.sqrt(u.astype(np.float64) ** 2 + v.astype(np.float64) ** 2)
    assert (ok[r > 1.001] == 0).all() and (ok[r < 0.999] == 1).all()
    assert np.isfinite(d[ok == 1]).all()
