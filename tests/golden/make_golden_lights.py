#!/usr/bin/env python3
"""Records tests/golden/lights_ext.npz: the scenes of tests/lightslib.py rendered by the reference
library itself (the CPU oracle has no spot, directional, sun or sphere light).

    cmake -S <reference> -B <dir> -G Ninja -DCMAKE_BUILD_TYPE=Release && ninja -C <dir>
    python tests/golden/make_golden_lights.py <dir>/src/libyafaray4.so

The reference's libyafaray4.so is loaded with ctypes and scenes.apply(spec, api) is replayed on it through
an `api` object that differs from libyafaray_amd.Interface in three points: the vertices and triangles go
through yafaray_addVertex / yafaray_addTriangle (the reference has no bulk calls), the put-pixel callback
is registered before yafaray_setupRender, and the combined layer is an exported one (the reference hands
only exported layers to the callback).  Every scene is rendered twice and must repeat bit for bit.
Never run by a test: the tests only read the file."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import dataclasses  # noqa: E402

import lightslib  # noqa: E402
from libyafaray_amd import scenes  # noqa: E402

PutPixelCb = C.CFUNCTYPE(None, C.c_char_p, C.c_char_p, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p)
ProgressCb = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_char_p, C.c_void_p)


def _b(s):
    return s.encode() if isinstance(s, str) else s


class RefApi:
    """The subset of libyafaray_amd.Interface that scenes.apply() uses, on the reference library."""

    def __init__(self, path, width, height):
        L = self.L = C.CDLL(path)
        vp, cp, i, d, f = C.c_void_p, C.c_char_p, C.c_int, C.c_double, C.c_float
        sig = {
            "yafaray_createInterface": (vp, [i, cp, vp, vp, i]),
            "yafaray_destroyInterface": (None, [vp]),
            "yafaray_setConsoleVerbosityLevel": (None, [vp, i]),
            "yafaray_setLogVerbosityLevel": (None, [vp, i]),
            "yafaray_createScene": (None, [vp]),
            "yafaray_endObject": (i, [vp]),
            "yafaray_addVertex": (i, [vp, d, d, d]),
            "yafaray_addTriangle": (i, [vp, i, i, i]),
            "yafaray_paramsSetVector": (None, [vp, cp, d, d, d]),
            "yafaray_paramsSetString": (None, [vp, cp, cp]),
            "yafaray_paramsSetBool": (None, [vp, cp, i]),
            "yafaray_paramsSetInt": (None, [vp, cp, i]),
            "yafaray_paramsSetFloat": (None, [vp, cp, d]),
            "yafaray_paramsSetColor": (None, [vp, cp, f, f, f, f]),
            "yafaray_paramsClearAll": (None, [vp]),
            "yafaray_setCurrentMaterial": (None, [vp, cp]),
            "yafaray_createObject": (i, [vp, cp]),
            "yafaray_createLight": (i, [vp, cp]),
            "yafaray_createMaterial": (i, [vp, cp]),
            "yafaray_createCamera": (i, [vp, cp]),
            "yafaray_createBackground": (i, [vp, cp]),
            "yafaray_createIntegrator": (i, [vp, cp]),
            "yafaray_createRenderView": (i, [vp, cp]),
            "yafaray_setRenderPutPixelCallback": (None, [vp, PutPixelCb, vp]),
            "yafaray_setupRender": (None, [vp]),
            "yafaray_render": (None, [vp, ProgressCb, vp, i]),
            "yafaray_defineLayer": (None, [vp]),
        }
        for name, (res, args) in sig.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
        # REF_VERBOSITY=4 (info) shows the reference's log on the console, "New scene bound is" in it
        verbosity = int(os.environ.get("REF_VERBOSITY", "0"))
        self.h = L.yafaray_createInterface(0, None, None, None, 1 if verbosity else 0)
        L.yafaray_setConsoleVerbosityLevel(self.h, verbosity)
        L.yafaray_setLogVerbosityLevel(self.h, 0)
        self.img = np.full((height, width, 4), np.nan, np.float32)
        self._last = {}

        def put(view, layer, x, y, r, g, b, a, data):
            if layer == b"combined":
                self.img[y, x] = (r, g, b, a)
        self._cb = PutPixelCb(put)
        self._pcb = ProgressCb(lambda t, dn, tag, d: None)

    def __getattr__(self, name):
        fn = getattr(self.L, "yafaray_" + name)

        def call(*args):
            return fn(self.h, *[_b(a) for a in args])
        return call

    def paramsSetString(self, k, v):
        self._last[k] = v
        self.L.yafaray_paramsSetString(self.h, _b(k), _b(v))

    def paramsClearAll(self):
        self._last = {}
        self.L.yafaray_paramsClearAll(self.h)

    def addVertices(self, xyz):
        for v in np.asarray(xyz, np.float64).reshape(-1, 3):
            self.L.yafaray_addVertex(self.h, float(v[0]), float(v[1]), float(v[2]))

    def addTriangles(self, abc):
        for t in np.asarray(abc, np.int32).reshape(-1, 3):
            self.L.yafaray_addTriangle(self.h, int(t[0]), int(t[1]), int(t[2]))

    def defineLayer(self):
        if self._last.get("type") == "combined" and "exported_image_type" not in self._last:
            self.paramsSetString("exported_image_type", "ColorAlpha")
            self.paramsSetString("exported_image_name", "Combined")
        self.L.yafaray_defineLayer(self.h)

    def setupRender(self):
        self.L.yafaray_setRenderPutPixelCallback(self.h, self._cb, None)
        self.L.yafaray_setupRender(self.h)

    def createLight(self, name):
        if not self.L.yafaray_createLight(self.h, _b(name)):
            raise RuntimeError("the reference refused light '%s'" % name)
        return 1

    def render(self):
        self.L.yafaray_render(self.h, self._pcb, None, 0)
        return self.img

    def close(self):
        self.L.yafaray_destroyInterface(self.h)


def render_reference(path, spec):
    api = RefApi(path, spec.render.width, spec.render.height)
    scenes.apply(spec, api)
    img = api.render().copy()
    api.close()
    return img


def light_params(spec):
    return [{k: (list(v) if isinstance(v, tuple) else v) for k, v in dataclasses.asdict(l).items()} for l in spec.lights]


def main():
    path = os.path.abspath(sys.argv[1])
    only = sys.argv[2:]
    out = {}
    params = {}
    for name in only or lightslib.names():
        spec = lightslib.spec(name)
        a = render_reference(path, spec)
        b = render_reference(path, spec)
        assert np.isfinite(a).all(), name + ": not finite (or a pixel never delivered)"
        assert a.tobytes() == b.tobytes(), name + ": the reference does not repeat"
        assert a[..., :3].max() > 0, name + ": black"
        out[name] = a
        params[name] = {"integrator": spec.render.integrator, "lights": light_params(spec)}
        print("%-12s mean %.6f max %.6f lit %d" % (name, a[..., :3].mean(), a[..., :3].max(), int((a[..., :3].sum(-1) > 0).sum())), flush=True)
    if only:
        return
    out["params_json"] = np.frombuffer(json.dumps(params, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(HERE, "lights_ext.npz")
    np.savez_compressed(dst, **out)
    print(dst, os.path.getsize(dst), "bytes")


if __name__ == "__main__":
    main()
