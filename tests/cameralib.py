"""The scenes of tests/golden/cameras.npz: the small Cornell box through the architect, orthographic,
equirectangular and angular cameras (and through the control's perspective camera), under the three integrators,
with render layers, and the specular recursion tree under two of them.

Shared by the generator (tests/golden/make_golden_cameras.py, which records the reference library's pixels)
and by the tests that compare against the record.

Every camera aims slightly off the box's axes: an orthographic bundle parallel to the walls, or a view direction in
a plane of symmetry, meets the quads' shared diagonals and the box edges at exact-t ties, which the reference's
kd-tree and this BVH may settle differently (the reason lightslib.spec("tree_dl") lifts the boxes)."""
import dataclasses
import os

import numpy as np

import layerlib
import lightslib
from libyafaray_amd import scenes
from libyafaray_amd.scenes import Light

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "cameras.npz")

W, H = 48, 36
EQUI_W, EQUI_H = 48, 24
CONTROL = "control_dl"
INTEGRATORS = lightslib.INTEGRATORS
LAYERS = ["z-depth-abs", "debug-uv", "debug-normal-smooth"]
PROJECTIONS = ("equidistant", "orthographic", "stereographic", "equisolid_angle", "rectilinear")

ulp_distance = lightslib.ulp_distance
bad_pixels = lightslib.bad_pixels


def _up(from_):
    return (from_[0], from_[1], from_[2] + 1.0)


def _cam(type_, from_, to, w=W, h=H, **kw):
    return scenes.Camera(from_=from_, to=to, up=_up(from_), resx=w, resy=h, type=type_, **kw)


# outside the open front, the whole box in view: 2.9 wide, 2.175 high
ORTHO = dict(from_=(0.03, -3.9, 1.02), to=(0.07, 0.0, 0.98), scale=2.9)
# inside the box, looking at the back wall
INSIDE = dict(from_=(0.11, -0.62, 1.07), to=(0.16, 0.4, 1.01))

CAMERAS = {
    "ortho": _cam("orthographic", **ORTHO),
    # the planes cut through the box: it spans distances 2.9 .. 4.9 from the camera
    "ortho_clip": _cam("orthographic", near_clip=3.45, far_clip=4.35, **ORTHO),
    "equi": _cam("equirectangular", w=EQUI_W, h=EQUI_H, **INSIDE),
    # a far plane: through the open front a miss keeps the ray's tmax, which the type's own far plane (-1.0e38) over a
    # small cosine takes to infinity, and the absolute-depth layer shows it
    "equi_layers": _cam("equirectangular", w=EQUI_W, h=EQUI_H, far_clip=12.0, **INSIDE),
    "ang_square_layers": _cam("angular", angle=90.0, circular=False, mirrored=True, far_clip=12.0, **INSIDE),
    "ang_max": _cam("angular", angle=90.0, max_angle=70.0, **INSIDE),
    "ang_square": _cam("angular", angle=90.0, circular=False, mirrored=True, **INSIDE),
    # tilted down, so that the architect's vertical differs from the camera's
    "arch": _cam("architect", from_=(0.05, -3.9, 1.7), to=(0.09, 0.0, 0.8), focal=1.4),
    "arch_dof": _cam("architect", from_=(0.05, -3.9, 1.7), to=(0.09, 0.0, 0.8), focal=1.4, aperture=0.08, dof_distance=3.9,
                     bokeh_type="hexagon", bokeh_rotation=15.0),
}
# beyond the issue's list: 140 degrees each way look out of the open front, onto a coloured transparent background, so
# that a miss (alpha 0) and a sample without a ray (black, alpha 1) differ
CAMERAS["ang_wide_bg"] = _cam("angular", angle=140.0, **INSIDE)
for _p in PROJECTIONS:
    CAMERAS["ang_" + _p] = _cam("angular", angle=60.0 if _p == "rectilinear" else 90.0, projection=_p, **INSIDE)
for _k in ("ang_gauss", "ang_aa", "ang_two_lights"):
    CAMERAS[_k] = CAMERAS["ang_equidistant"]

TREE = ("ang_tree_dl", "ortho_tree_dl")
LAYERED = ("ortho_layers", "equi_layers", "ang_square_layers")


def _base(integrator, w=W, h=H):
    s = scenes.cornell(w, h, spp=2, bounces=3, rr=False, integrator=integrator)
    if integrator == "photonmapping":
        s = s.with_render(pm_photons=20000, pm_search=50, pm_diffuse_radius=0.1, pm_bounces=4, pm_final_gather=False,
                          threads_photons=1)
    return s


def spec(name):
    """The SceneSpec of a recorded scene."""
    if name == CONTROL:
        return lightslib.spec("bulb_dl")
    if name in TREE:
        s = lightslib.spec(lightslib.TREE)   # the lifted boxes
        s = dataclasses.replace(s, lights=scenes.cornell_specular(W, H).lights)
        return dataclasses.replace(s, camera=CAMERAS["ang_equidistant" if name == "ang_tree_dl" else "ortho"])
    which, kind = name.rsplit("_", 1)
    cam = CAMERAS.get(name, CAMERAS.get(which))
    s = _base(INTEGRATORS.get(kind, "directlighting"), cam.resx, cam.resy)
    s = dataclasses.replace(s, camera=cam)
    if kind == "layers":
        s = dataclasses.replace(s, layers=[layerlib.layer(t) for t in layer_names(name)])
    if which == "ang_gauss":
        s = s.with_render(filter_type="gauss", aa_pixelwidth=1.5)
    if which == "ang_aa":
        s = s.with_render(aa_passes=2)
    if which == "ang_wide_bg":
        s = dataclasses.replace(s.with_render(bg_transp=True), background=scenes.Background((0.2, 0.3, 0.5), 1.0))
    if which == "ang_two_lights":
        s = dataclasses.replace(s, lights=scenes.with_extra_lights(s, 2).lights)
    return s


def names():
    out = [CONTROL, "ortho_dl", "ortho_pt", "ortho_pm", "ortho_clip_dl", "equi_dl", "equi_pt", "equi_pm"]
    out += ["ang_%s_dl" % p for p in PROJECTIONS]
    out += ["ang_equidistant_pt", "ang_max_dl", "ang_square_dl", "ang_gauss_dl", "ang_aa_dl", "ang_two_lights_pt", "ang_wide_bg_dl",
            "arch_dl", "arch_dof_pt"]
    return out + list(LAYERED) + list(TREE)


def circular_names():
    """The scenes whose camera gives no ray outside a circle: their corners are the film's default colour."""
    return [n for n in names() if spec(n).camera.type == "angular" and spec(n).camera.circular]


def layer_names(name):
    """The layers recorded beside "combined" for a scene, in the fixture's key order."""
    if name == "ortho_layers":
        # beyond the issue's list: the normalised depth, whose range comes from the depth pre-pass's own rays
        return LAYERS + ["z-depth-norm"]
    return LAYERS if name in LAYERED else []


def camera_params(s):
    return {k: (list(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(s.camera).items()}


def corners(img):
    """The four corner pixels."""
    return np.stack([img[0, 0], img[0, -1], img[-1, 0], img[-1, -1]])


_fixture = None


def fixture():
    """The recorded pixels, loaded once and shared (read-only arrays)."""
    global _fixture
    if _fixture is None:
        with np.load(FIXTURE) as z:
            _fixture = {k: z[k] for k in z.files}
        for v in _fixture.values():
            v.setflags(write=False)
    return _fixture
