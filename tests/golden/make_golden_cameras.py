#!/usr/bin/env python3
"""Records tests/golden/cameras.npz: the scenes of tests/cameralib.py rendered by the reference library itself
(the CPU oracle has the perspective camera alone).

    cmake -S <reference> -B <dir> -G Ninja -DCMAKE_BUILD_TYPE=Release && ninja -C <dir>
    python tests/golden/make_golden_cameras.py <dir>/src/libyafaray4.so

RefApi of make_golden_lights.py replays scenes.apply(spec, api) on the reference's libyafaray4.so; here its
put-pixel callback also keeps the exported layers beside "combined" (keys "<scene>/<layer type>").  Every scene is
rendered twice and must repeat bit for bit.  Never run by a test: the tests only read the file."""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import make_golden_lights as G  # noqa: E402  (puts the repository root and tests/ on sys.path)

import cameralib  # noqa: E402
from libyafaray_amd import scenes  # noqa: E402

MAX_BYTES = 1 << 20


class RefApiLayers(G.RefApi):
    """RefApi whose callback keeps every exported layer: self.layers[<layer type>] = (h, w, 4) float32."""

    def __init__(self, path, width, height):
        super().__init__(path, width, height)
        self.layers = {}

        def put(view, layer, x, y, r, g, b, a, data):
            name = layer.decode()
            if name == "combined":
                self.img[y, x] = (r, g, b, a)
            else:
                if name not in self.layers:
                    self.layers[name] = np.full((height, width, 4), np.nan, np.float32)
                self.layers[name][y, x] = (r, g, b, a)
        self._cb = G.PutPixelCb(put)

    def paramsSetInt(self, k, v):
        # one render thread: with a filter wider than a pixel the tiles add to each other's pixels, and the sums
        # depend on the order in which the threads finish (ang_gauss_dl does not repeat otherwise)
        self.L.yafaray_paramsSetInt(self.h, G._b(k), 1 if k == "threads" else int(v))


def render_reference(path, spec):
    api = RefApiLayers(path, spec.render.width, spec.render.height)
    scenes.apply(spec, api)
    img = api.render().copy()
    layers = {k: v.copy() for k, v in api.layers.items()}
    api.close()
    return img, layers


def main():
    path = os.path.abspath(sys.argv[1])
    only = sys.argv[2:]
    out = {}
    params = {}
    circular = set(cameralib.circular_names())
    for name in only or cameralib.names():
        spec = cameralib.spec(name)
        a, la = render_reference(path, spec)
        b, lb = render_reference(path, spec)
        assert np.isfinite(a).all(), name + ": not finite (or a pixel never delivered)"
        assert a.tobytes() == b.tobytes(), name + ": the reference does not repeat"
        assert a[..., :3].max() > 0, name + ": black"
        assert sorted(la) == sorted(cameralib.layer_names(name)), (name, sorted(la))
        for k in la:
            assert np.isfinite(la[k]).all() and la[k].tobytes() == lb[k].tobytes(), name + "/" + k
            out[name + "/" + k] = la[k]
        surround = int(((a == np.float32([0, 0, 0, 1])).all(-1)).sum())
        seen = int(((a[..., 3] < 1) | (a[..., :3].sum(-1) > 0)).sum())
        if name in circular:
            assert surround > 0 and seen > 0, (name, surround, seen)
            # (a wide filter's normalised alpha is a rounded sum / sum: one only up to a few ULP)
            c = cameralib.corners(a)
            assert (c[:, :3] == 0).all() and (np.abs(c[:, 3] - 1) < 1e-6).all(), name + ": a corner inside the circle"
        out[name] = a
        params[name] = {"integrator": spec.render.integrator, "camera": cameralib.camera_params(spec)}
        print("%-22s mean %.6f max %.6f lit %4d black-opaque %4d alpha<1 %4d" %
              (name, a[..., :3].mean(), a[..., :3].max(), int((a[..., :3].sum(-1) > 0).sum()), surround, int((a[..., 3] < 1).sum())), flush=True)
    if only:
        return
    out["params_json"] = np.frombuffer(json.dumps(params, sort_keys=True).encode(), np.uint8)
    dst = os.path.join(HERE, "cameras.npz")
    np.savez_compressed(dst, **out)
    size = os.path.getsize(dst)
    print(dst, size, "bytes")
    assert size <= MAX_BYTES, size


if __name__ == "__main__":
    main()
