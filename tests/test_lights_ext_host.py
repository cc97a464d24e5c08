"""Spot, directional, sun and sphere lights at the C API, and the recorded reference pixels they are tested
against (tests/golden/lights_ext.npz, made by tests/golden/make_golden_lights.py from the reference library;
the CPU oracle has none of these lights).  No GPU needed."""
import numpy as np
import pytest

import lightslib as LL
from libyafaray_amd import scenes

DEFAULTS = [("spotlight", {}), ("directional", {}), ("sunlight", {}), ("spherelight", {})]
FULL = [
    ("spotlight", {"from": ("v", (0.6, -0.8, 1.9)), "to": ("v", (0.0, 0.0, 0.3)), "color": ("c", (1.0, 0.9, 0.8, 1.0)), "power": ("f", 8.0),
                   "cone_angle": ("f", 30.0), "blend": ("f", 0.3), "soft_shadows": ("b", False), "samples": ("i", 8),
                   "shadowFuzzyness": ("f", 1.0), "light_enabled": ("b", True), "cast_shadows": ("b", False),
                   "with_caustic": ("b", False), "with_diffuse": ("b", True), "photon_only": ("b", False)}),
    ("directional", {"direction": ("v", (0.1, -1.0, 0.2)), "infinite": ("b", False), "from": ("v", (0.0, -2.5, 1.2)), "radius": ("f", 0.6),
                     "color": ("c", (0.7, 0.8, 1.0, 1.0)), "power": ("f", 2.0), "cast_shadows": ("b", True), "photon_only": ("b", True)}),
    ("directional", {"direction": ("v", (0.1, -1.0, 0.2)), "infinite": ("b", False), "position": ("v", (0.0, -2.5, 1.2))}),
    ("sunlight", {"direction": ("v", (-0.3, -1.0, 0.5)), "angle": ("f", 95.0), "samples": ("i", 2), "power": ("f", 1.5),
                  "with_caustic": ("b", True), "with_diffuse": ("b", False)}),
    ("spherelight", {"from": ("v", (0.3, -0.2, 1.5)), "radius": ("f", 0.12), "samples": ("i", 2), "power": ("f", 4.0),
                     "object_name": ("s", "nothing"), "light_enabled": ("b", False)}),
]


def _create(product, ltype, params):
    yi = product.Interface()
    yi.createScene()
    yi.paramsClearAll()
    yi.paramsSetString("type", ltype)
    for k, tv in params.items():
        scenes.set_typed(yi, k, tv)
    ok = yi.createLight("l")
    err = yi.last_error()
    yi.close()
    return ok, err


@pytest.mark.parametrize("ltype,params", DEFAULTS + FULL, ids=lambda v: v if isinstance(v, str) else "-".join(sorted(v))[:40])
def test_create_light_accepts_the_four_types(product, ltype, params):
    ok, err = _create(product, ltype, params)
    assert ok == 1, err
    assert "not supported" not in err


@pytest.mark.parametrize("ltype,params", [("spotlight", {"soft_shadows": ("b", True)}), ("ies", {}), ("bglight", {})],
                         ids=["spot_soft_shadows", "ies", "bglight"])
def test_create_light_still_refuses(product, ltype, params):
    ok, err = _create(product, ltype, params)
    assert ok == 0
    assert "not supported by the GPU core" in err


@pytest.mark.parametrize("name", LL.names())
def test_recorded_specs_stage(product, name):
    spec = LL.spec(name)
    yi = product.Interface()
    scenes.apply(spec, yi)
    err = yi.last_error()
    w, h = yi.getSceneFilmWidth(), yi.getSceneFilmHeight()
    yi.close()
    assert err == ""
    assert (w, h) == (LL.W, LL.H)


def test_existing_specs_issue_the_calls_they_issued():
    """A point, area or mesh light sets none of the new parameters."""
    class Rec:
        def __init__(self):
            self.calls = []

        def __getattr__(self, name):
            def call(*a):
                self.calls.append((name,) + tuple(x if not isinstance(x, np.ndarray) else x.tobytes() for x in a))
                return 1
            return call
    new_keys = {"to", "cone_angle", "blend", "direction", "infinite", "radius", "angle"}
    for spec in (scenes.with_extra_lights(scenes.cornell(16, 12), 3), scenes.cornell_meshlight(16, 12, keep_area=True)):
        r = Rec()
        scenes.apply(spec, r)
        keys, lights = set(), 0
        for c in r.calls:
            if c[0] == "paramsClearAll":
                keys = set()
            elif c[0].startswith("paramsSet"):
                keys.add(c[1])
            elif c[0] == "createLight":
                lights += 1
                assert not (keys & new_keys), keys & new_keys
        assert lights == len(spec.lights)


def test_fixture_has_every_scene():
    fx = LL.fixture()
    imgs = {}
    for name in LL.names():
        assert name in fx, name
        a = fx[name]
        assert a.shape == (LL.H, LL.W, 4) and a.dtype == np.float32
        assert np.isfinite(a).all(), name
        assert a[..., :3].max() > 0, name
        imgs[name] = a.tobytes()
    assert len(set(imgs.values())) == len(imgs), "two recorded scenes are equal"
    assert "params_json" in fx


@pytest.mark.parametrize("name", LL.control_names())
def test_oracle_equals_the_record_on_the_control_scenes(oracle_built, name):
    """The recorded control scenes (a point light) are scenes the CPU oracle renders: it must equal the
    reference's recorded pixels exactly, which validates the generator and the comparison."""
    rgba, _, _ = oracle_built.OracleScene(LL.spec(name), threads=4).render()
    d = LL.ulp_distance(rgba, LL.fixture()[name])
    assert int(d.max()) == 0, (int(d.max()), int((d > 0).sum()))
