"""The scenes of tests/golden/lights_ext.npz: the small Cornell box lit by one spot, directional, sun or
sphere light (or by the control point light), under the three integrators, and two scenes with all of them.

Shared by the generator (tests/golden/make_golden_lights.py, which records the reference library's pixels)
and by the tests that compare against the record."""
import dataclasses
import os

import numpy as np

from libyafaray_amd import scenes
from libyafaray_amd.scenes import Light

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "lights_ext.npz")

W, H = 48, 36

LIGHTS = {
    "spot": Light("spot", type="spotlight", from_=(0.6, -0.8, 1.9), to=(0.0, 0.0, 0.3), cone_angle=30.0, blend=0.3,
                  power=8.0, color=(1.0, 0.9, 0.8)),
    "dir_inf": Light("dir_inf", type="directional", direction=(0.2, -1.0, 0.4), infinite=True, power=1.5),
    "dir_cyl": Light("dir_cyl", type="directional", direction=(0.1, -1.0, 0.2), infinite=False, from_=(0.0, -2.5, 1.2),
                     radius=0.6, power=2.0, color=(0.7, 0.8, 1.0)),
    "sun": Light("sun", type="sunlight", direction=(-0.3, -1.0, 0.5), angle=3.0, samples=2, power=1.5),
    "ball": Light("ball", type="spherelight", from_=(0.3, -0.2, 1.5), radius=0.12, samples=2, power=4.0),
}
NEW = ("spot", "dir_inf", "dir_cyl", "sun", "ball")
CONTROL = "bulb"
INTEGRATORS = {"dl": "directlighting", "pt": "pathtracing", "pm": "photonmapping"}


def _base(integrator):
    s = scenes.cornell(W, H, spp=2, bounces=3, rr=False, integrator=integrator)
    if integrator == "photonmapping":
        s = s.with_render(pm_photons=20000, pm_search=50, pm_diffuse_radius=0.1, pm_bounces=4, pm_final_gather=False,
                          threads_photons=1)
    return s


def _bulb():
    return scenes.with_extra_lights(scenes.cornell(W, H), 2).lights[1]


TREE = "tree_dl"   # beyond the issue's list: the new lights under the specular recursion tree and shader-node kernels


def spec(name):
    """The SceneSpec of a recorded scene: "<light>_<dl|pt|pm>", "all_dl", "all_pm" or "tree_dl" (direct lighting
    of scenes.cornell_specular, whose mirror, Fresnel and transparent materials spawn recursion-tree nodes, lit
    by the five new lights)."""
    if name == TREE:
        s = scenes.cornell_specular(W, H, spp=2, integrator="directlighting", raydepth=3)
        # the boxes are lifted off the floor: a ray refracted through the transparent box would otherwise meet its
        # bottom face and the floor at exactly the same t, a tie that the reference's kd-tree and a BVH settle
        # differently (with the box's own area light as well)
        verts = s.verts.copy()
        for o in s.objects:
            if o.name in ("short_box", "tall_box"):
                verts[o.v0:o.v0 + o.nv, 2] += np.float32(1.0 / 64.0)
        return dataclasses.replace(s, verts=verts, lights=[LIGHTS[k] for k in NEW])
    which, integ = name.rsplit("_", 1)
    s = _base(INTEGRATORS[integ])
    if which == "all":
        lights = [LIGHTS[k] for k in NEW] + list(s.lights)
    elif which == CONTROL:
        lights = [_bulb()]
    else:
        lights = [LIGHTS[which]]
    return dataclasses.replace(s, lights=lights)


def names():
    out = ["%s_%s" % (l, i) for l in NEW + (CONTROL,) for i in INTEGRATORS]
    return out + ["all_dl", "all_pm", TREE]


def control_names():
    return ["%s_%s" % (CONTROL, i) for i in INTEGRATORS]


def ulp_distance(a, b):
    """Per value: the number of float32 steps between a and b (both finite)."""
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)

    def key(x):
        i = x.view(np.int32).astype(np.int64)
        return np.where(i < 0, -(i & 0x7FFFFFFF), i)
    return np.abs(key(a) - key(b))


def bad_pixels(img, ref, ulp=4):
    """Pixels with any of their values further than `ulp` float32 steps from the record."""
    return int(np.count_nonzero((ulp_distance(img, ref) > ulp).any(axis=-1)))


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
