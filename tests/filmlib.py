"""Film filter test support: the product's host film set-up (tests/hostmath_host.cc over hostmath.h), scenes whose
samples are exact on both sides, and a plain numpy restatement of ImageFilm::addSample (imagefilm.cc:680-733)."""
import ctypes as C
import dataclasses
import os
import subprocess
import tempfile

import numpy as np

from libyafaray_amd import scenes

HERE = os.path.dirname(os.path.abspath(__file__))
FILTERS = {"box": 0, "gauss": 1, "mitchell": 2, "lanczos": 3}
_host = None


def host():
    """hostmath.h built for the test (g++ -O2 -ffp-contract=off, as devmath_host.cc)."""
    global _host
    if _host is None:
        out = os.path.join(tempfile.gettempdir(), "yaf_hostmath_host_%d.so" % os.getuid())
        subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                        os.path.join(HERE, "hostmath_host.cc")], check=True)
        _host = C.CDLL(out)
    return _host


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def host_filter(name, dxdy):
    """hm::filterBox / filterGauss / filterMitchell / filterLanczos at (dx, dy) pairs."""
    d = np.ascontiguousarray(dxdy, np.float32).reshape(-1)
    out = np.empty(len(d) // 2, np.float32)
    host().hmh_filter(FILTERS[name], _p(d, C.c_float), _p(out, C.c_float), len(out))
    return out


@dataclasses.dataclass
class Setup:
    table: np.ndarray      # (256,) float32, row dy, column dx
    filterw: float         # float32 values held in Python floats
    table_scale: float
    reach_fwd: int         # a pixel's sources lie in [x - reach_fwd, x + reach_back]
    reach_back: int


def film_setup(name, pixelwidth):
    """hm::filmSetup: what host.cc hands to the film kernels for (filter, AA_pixelwidth)."""
    tab = np.empty(256, np.float32)
    fw, ts, reach = C.c_float(), C.c_float(), (C.c_int * 2)()
    host().hmh_film_setup(FILTERS[name], C.c_float(pixelwidth), _p(tab, C.c_float), C.byref(fw), C.byref(ts), reach)
    return Setup(tab, fw.value, ts.value, reach[0], reach[1])


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


EMIT = (0.5, 1.25, 2.0)   # white, red, green: exactly representable strengths


def exact_scene(W, H, spp, **render):
    """The Cornell geometry as three emitters and no lights under direct lighting: every sample's colour is
    emit x colour of the closest hit (or the black background), one float product on either side, so the
    samples are bit-identical by construction and only the film arithmetic is compared."""
    s = scenes.cornell(W, H, spp=spp, bounces=1, integrator="directlighting")
    mats = [dataclasses.replace(m, emit=e) for m, e in zip(s.materials, EMIT)]
    return dataclasses.replace(s, materials=mats, lights=[]).with_render(**render)


def tile_list(W, H, ts, order):
    """Tiles in render order as (x0, y0, x1, y1): linear, or centre with ties in linear order (imagesplitter.cc:30-107;
    pinned against the oracle's lists by tests/test_tiles_order.py)."""
    ntx, nty = (W + ts - 1) // ts, (H + ts - 1) // ts
    ids = list(range(ntx * nty))
    if order == "centre":
        ids.sort(key=lambda i: ((i % ntx) * ts - W // 2) ** 2 + ((i // ntx) * ts - H // 2) ** 2)
    elif order != "linear":
        raise ValueError(order)
    return [((i % ntx) * ts, (i // ntx) * ts, min(W, (i % ntx) * ts + ts), min(H, (i // ntx) * ts + ts)) for i in ids]


def _round_to_int(v):
    return int(v + (.5 - 1.4e-11))     # math.h roundToInt: truncation of v + (0.5 - 1.4e-11)


def normalized(acc, wt):
    """Rgba::normalized (color.h:554-558): colour x (1 / weight), zero where the weight is zero."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.float32(1.0) / wt
        return np.where((wt != 0)[..., None], acc * inv[..., None], np.float32(0.0)).astype(np.float32)


def splat(samples, tiles, setup, dx=0.5, dy=0.5):
    """ImageFilm::addSample over a one-sample-per-pixel image (H, W, 4): tiles in order, pixels row-major inside
    a tile, each sample at sub-pixel (dx, dy) added to every pixel of its footprint in float32.  Returns the
    normalised film after each tile (one (H, W, 4) array per tile) — the last is the final film — and the
    final weights."""
    H, W = samples.shape[:2]
    fw, scale = float(np.float32(setup.filterw)), float(np.float32(setup.table_scale))
    tab = setup.table.reshape(16, 16)
    acc, wt = np.zeros((H, W, 4), np.float32), np.zeros((H, W), np.float32)
    after = []
    for x0, y0, x1, y1 in tiles:
        for y in range(y0, y1):
            for x in range(x0, x1):
                dx_0, dx_1 = max(0 - x, _round_to_int(dx - fw)), min(W - x - 1, _round_to_int(dx + fw - 1.0))
                dy_0, dy_1 = max(0 - y, _round_to_int(dy - fw)), min(H - y - 1, _round_to_int(dy + fw - 1.0))
                if dx_0 > dx_1 or dy_0 > dy_1:
                    continue
                xi = [int(np.floor(abs((i - (dx - 0.5)) * scale))) for i in range(dx_0, dx_1 + 1)]
                yi = [int(np.floor(abs((j - (dy - 0.5)) * scale))) for j in range(dy_0, dy_1 + 1)]
                w = tab[np.ix_(yi, xi)]
                ys, xs = slice(y + dy_0, y + dy_1 + 1), slice(x + dx_0, x + dx_1 + 1)
                wt[ys, xs] = wt[ys, xs] + w
                acc[ys, xs] = acc[ys, xs] + samples[y, x][None, None, :] * w[..., None]
        after.append(normalized(acc, wt))
    return after, wt
