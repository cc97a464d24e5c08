"""devmath.h and texeval.h as compiled for gfx950, function by function and bit for bit.

tests/devmath_dev.hip puts every function family behind one plain kernel and is built by `make devcheck` with the
product's own device flags; each device result is compared as uint32 / uint64 with its named reference: the g++ host
build of the same header (tests/devmath_host.cc, itself pinned to real long double and to the host's libm by
tests/test_devmath.py), the reference's golden vectors (tests/golden/prims.npz, tex_prims.npz), or plain integer
arithmetic.  texeval.h cannot be built by g++; its functions also run in the host pass of the harness's own translation
unit, and the two passes are compared.  The only latitude anywhere is a NaN on both sides.

Inputs left out, because the reference's own behaviour is undefined there (a float -> int conversion of a NaN or of
|value| >= 2^31, where x86 and gfx950 legitimately differ): fsin / fcos inputs stay within |x| <= 1e9, and fmPow inputs
are finite with a > 0.  Nothing else is excluded, and no generated set is filtered."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np
import pytest

import devmathlib as L
from devmathlib import P

pytestmark = pytest.mark.gpu

GOLD = np.load(os.path.join(L.HERE, "golden", "prims.npz"))
TEX = np.load(os.path.join(L.HERE, "golden", "tex_prims.npz"))
f, u = C.c_float, C.c_uint32


@pytest.fixture(scope="module")
def dev():
    out = os.path.join(tempfile.mkdtemp(prefix="yaf_devcheck_"), "devmath_check.so")
    r = subprocess.run(["make", "-j16", "-C", os.path.join(L.ROOT, "libyafaray_amd", "csrc"), "devcheck", "DEVCHECK_OUT=" + out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return C.CDLL(out)


@pytest.fixture(scope="module")
def host():
    return L.host_lib()


def check(name, got, want, *inputs):
    ok = L.same_bits(got, want)
    assert ok.all(), L.describe(name, ok, got, want, *inputs)


def outs(n, k=2):
    return [np.empty(n, np.float32) for _ in range(k)]


# ---- x87 emulation ----
def x87_sets(dispatcher):
    """[(constant, operands)] of a dispatcher: the distributions of devmath_check.cc, the sphere grid, and the
    near-midpoint inputs of the binade scans."""
    d = L.x87_inputs()
    near, total = L.near_midpoint(dispatcher)
    print(f"{dispatcher}: {total} near-midpoint inputs")
    assert total >= L.NEAR_MIN, f"{dispatcher}: only {total} near-midpoint inputs found on the CPU"
    nargs = {"x87mul": 1, "x87mul2": 2, "x87mul3": 3, "x87mulDiv": 2, "x87recipMul": 1}[dispatcher]
    sets = [(c, (x, y, z)[:nargs]) for c, x, y, z in near]
    if dispatcher == "x87mul":
        wide = L.f32(np.concatenate([d["x"], d["s2"], L.sphere_inputs()]))
        sets += [(c, (wide,)) for c in (L.K_DIV_4_BY_PI, L.K_MULT_PI_BY_2, L.K_DIV_1_BY_PI)]
    elif dispatcher == "x87mul2":
        wide = L.f32(np.concatenate([d["x"], L.sphere_inputs()]))
        sets += [(L.K_DIV_4_BY_SQUARED_PI, (wide, np.abs(wide)))]
    elif dispatcher == "x87mul3":
        sets += [(L.K_DIV_1_BY_PI, L.kernel_inputs())]
    elif dispatcher == "x87mulDiv":
        sets += [(c, (d["a"], d["b"])) for c in (L.K_PI, L.K_MULT_PI_BY_2)]
    else:
        sets += [(L.K_PI, (d["pr"],))]
    return sets


def test_round64_round24(dev, host):
    """The two roundings of every exact path on double-doubles that reach their ties (see devmathlib.round_inputs),
    against the g++ build, whose results tests/test_devmath.py pins to real long double."""
    hi, lo = L.round_inputs()
    n = len(hi)
    d, h = C.c_double, [np.empty(n), np.empty(n), np.empty(n, np.float32)]
    g = [np.empty(n), np.empty(n), np.empty(n, np.float32)]
    ok64, ref24 = np.empty(n, np.int32), np.empty(n, np.float32)
    assert dev.dd_round(P(hi, d), P(lo, d), n, P(g[0], d), P(g[1], d), P(g[2], f)) == 0
    host.dm_round(P(hi, d), P(lo, d), n, P(h[0], d), P(h[1], d), P(h[2], f), P(ok64, C.c_int32), P(ref24, f))
    check("round64 hi", g[0], h[0], hi, lo)
    check("round64 lo", g[1], h[1], hi, lo)
    check("round24", g[2], h[2], hi, lo)
    check("round24 vs long double", g[2], ref24, hi, lo)


X87_FN = {"x87mul": "x87mul", "x87mul2": "x87mul2", "x87mul3": "x87mul3", "x87mulDiv": "x87muldiv", "x87recipMul": "x87recip"}


@pytest.mark.parametrize("dispatcher", list(X87_FN))
def test_x87_dispatchers_and_exact_paths(dev, host, dispatcher):
    """Each dispatcher and its *Exact function on every input, against the g++ build; the near-midpoint inputs are the
    ones for which safeToRound is false, so the dispatcher's own slow branch runs on the device."""
    for c, ops in x87_sets(dispatcher):
        ops = [L.f32(o) for o in ops]
        n = len(ops[0])
        ptrs = [P(o, f) for o in ops]
        d_disp, d_exact = outs(n)
        h_disp, h_exact, h_ld = outs(n, 3)
        assert getattr(dev, "dd_" + X87_FN[dispatcher])(c, *ptrs, P(d_disp, f), P(d_exact, f), n) == 0
        getattr(host, "dm_" + X87_FN[dispatcher])(c, *ptrs, P(h_disp, f), P(h_exact, f), P(h_ld, f), n)
        check(f"{dispatcher} (constant {c})", d_disp, h_disp, *ops)
        check(f"{dispatcher}Exact (constant {c})", d_exact, h_exact, *ops)


def test_x87_one_minus_2_mul(dev, host):
    a = L.sphere_inputs()
    d, h, ld = outs(len(a), 3)
    assert dev.dd_x87one_minus(L.K_DIV_1_BY_PI, P(a, f), P(d, f), len(a)) == 0
    host.dm_x87one_minus(L.K_DIV_1_BY_PI, P(a, f), P(h, f), P(ld, f), len(a))
    check("x87oneMinus2Mul", d, h, a)
    check("x87oneMinus2Mul vs long double", d, ld, a)


# ---- libm restatements ----
def test_libm_restatements(dev, host):
    y, x = L.libm_inputs()
    got = [np.empty(len(y), np.float32) for _ in L.LIBM_NAMES]
    assert dev.dd_libm_all(P(y, f), P(x, f), len(y), (L.F * 5)(*[P(o, f) for o in got])) == 0
    for (name, (_, libm)), d in zip(L.host_libm(host).items(), got):
        check(name + " vs the host's libm", d, libm, y, x)


# ---- FAST_TRIG, vectors ----
def test_trig_golden_and_random(dev, host):
    x = GOLD["trig_x"]
    s, c = outs(len(x))
    assert dev.dd_sincos(P(x, f), P(s, f), P(c, f), len(x)) == 0
    check("fsin", s, GOLD["sin"], x)
    check("fcos", c, GOLD["cos"], x)
    rng = np.random.default_rng(21)
    n = 500_000
    x = L.f32(np.concatenate([rng.uniform(-1e9, 1e9, n), rng.uniform(-1, 1, n) * 10.0 ** rng.uniform(-8, 9, n),
                              [0.0, -0.0, 1e9, -1e9, np.pi, -np.pi, 2 * np.pi, -2 * np.pi]]))
    assert np.abs(x).max() <= 1e9
    s, c = outs(len(x))
    hs, hc = outs(len(x))
    assert dev.dd_sincos(P(x, f), P(s, f), P(c, f), len(x)) == 0
    host.dm_sin(P(x, f), P(hs, f), len(x))
    host.dm_cos(P(x, f), P(hc, f), len(x))
    check("fsin vs g++", s, hs, x)
    check("fcos vs g++", c, hc, x)


def test_hemisphere_and_vectors(dev):
    nrv, s = np.ascontiguousarray(GOLD["hemi_nrv"]), np.ascontiguousarray(GOLD["hemi_s"])
    o = np.empty((len(s), 3), np.float32)
    assert dev.dd_hemi(P(nrv, f), P(s, f), P(o, f), len(s)) == 0
    check("cosHemisphere", o, GOLD["hemi"], nrv, s)
    cin = np.ascontiguousarray(GOLD["coords_in"])
    o = np.empty((len(cin), 6), np.float32)
    assert dev.dd_coords(P(cin, f), P(o, f), len(cin)) == 0
    check("coordsSystem", o, GOLD["coords"], cin)
    v = np.ascontiguousarray(GOLD["norm_in"])
    o = np.empty_like(v)
    assert dev.dd_normalize(P(v, f), P(o, f), len(v)) == 0
    check("normalize", o, GOLD["norm"], v)


# ---- samplers ----
@pytest.mark.parametrize("which,name", [(0, "riVdC"), (1, "riS"), (2, "riLp")])
def test_radical_inverses(dev, which, name):
    b, r = GOLD["ri_bits"], GOLD["ri_r"]
    o = np.empty(len(b), np.float32)
    assert dev.dd_ri(which, P(b, u), P(r, u), P(o, f), len(b)) == 0
    check(name, o, GOLD[name], b, r)


def test_fnv_and_mwc(dev):
    b = GOLD["fnv_in"]
    o = np.empty(len(b), np.uint32)
    assert dev.dd_fnv(P(b, u), P(o, u), len(b)) == 0
    check("fnv32", o, GOLD["fnv"], b)
    seeds, ref = np.ascontiguousarray(GOLD["mwc_seeds"]), np.ascontiguousarray(GOLD["mwc"])
    o = np.empty_like(ref)
    assert dev.dd_mwc(P(seeds, u), ref.shape[1], P(o, C.c_double), len(seeds)) == 0
    check("Mwc", o, ref, seeds)


def test_bit_reverse(dev, host):
    rng = np.random.default_rng(3)
    edges = [0, 1, 2, 0x80000000, 0x40000000, 0xffffffff, 0xfffffffe, 0x7fffffff, 0x55555555, 0xaaaaaaaa, 0x0000ffff, 0xffff0000,
             0x00ff00ff, 0x0f0f0f0f, 0x33333333] + [1 << k for k in range(32)]
    v = np.ascontiguousarray(np.concatenate([np.arange(65536), rng.integers(0, 2 ** 32, 1_000_000), edges]).astype(np.uint32))
    d, h = np.empty_like(v), np.empty_like(v)
    assert dev.dd_bitrev(P(v, u), P(d, u), len(v)) == 0
    host.dm_bitrev(P(v, u), P(h, u), len(v))
    # the portable branch, once more without the header: reverse the bytes' bits through a table, and the bytes
    table = np.array([int(f"{i:08b}"[::-1], 2) for i in range(256)], np.uint8)
    plain = np.ascontiguousarray(table[v.view(np.uint8).reshape(-1, 4)][:, ::-1]).view(np.uint32).ravel()
    assert np.array_equal(h, plain)
    check("bitReverse32", d, h, v)


def test_magic_division(dev):
    for d, nn in L.udiv_cases():
        o = np.empty_like(nn)
        assert dev.dd_udiv(u(d), P(nn, u), P(o, u), len(nn)) == 0
        check(f"udiv by {d}", o, (nn.astype(np.uint64) // d).astype(np.uint32), nn)


def test_low_discrepancy_faure(dev):
    primes = L.primes_table()
    dims, idx, ref = GOLD["lds_dim"], GOLD["lds_idx"], GOLD["lds"]
    for d in np.unique(dims):
        m = dims == d
        pt = np.array(L.faure_perm(3 if d <= 2 else primes[d]), np.uint8)
        pt = np.ascontiguousarray(np.concatenate([pt, np.zeros(max(0, primes[d] - len(pt)), np.uint8)]))
        ii = np.ascontiguousarray(idx[m])
        o = np.empty(len(ii), np.float64)
        assert dev.dd_lds(P(pt, C.c_uint8), u(primes[d]), C.c_double(round(1e9 / primes[d]) / 1e9), P(ii, u), P(o, C.c_double),
                          len(ii)) == 0
        check(f"lowDiscrepancy dimension {d}", o, np.ascontiguousarray(ref[m]), ii)


def test_halton(dev, host):
    bases, starts, seq = GOLD["halton_bases"], GOLD["halton_starts"], GOLD["halton_seq"]
    assert seq.shape[1] == L.HALTON_K
    for base in np.unique(bases):
        m = bases == base
        st, first, nxt, inc = L.halton(dev.dd_halton, base, starts[m])
        assert st == 0
        want = np.ascontiguousarray(seq[m])
        check(f"haltonNext base {base}", nxt, want, starts[m])
        check(f"HaltonInc<{base}>", inc, want, starts[m])
        check(f"haltonFirst base {base}", first, np.ascontiguousarray(want[:, 0]), starts[m])
    rnd = np.random.default_rng(5).integers(0, 2 ** 32, 100_000, dtype=np.uint64).astype(np.uint32)
    for base in (2, 3, 5):
        st, first, nxt, inc = L.halton(dev.dd_halton, base, rnd)
        assert st == 0
        check(f"HaltonInc<{base}> vs haltonNext", inc, nxt, rnd)
        check(f"haltonFirst vs haltonNext, base {base}", first, np.ascontiguousarray(nxt[:, 0]), rnd)
        _, hfirst, hnxt, hinc = L.halton(host.dm_halton, base, rnd)
        check(f"haltonNext base {base} vs g++", nxt, hnxt, rnd)
        check(f"HaltonInc<{base}> vs g++", inc, hinc, rnd)
        check(f"haltonFirst base {base} vs g++", first, hfirst, rnd)


# ---- texeval.h ----
def test_fm_pow(dev):
    ab = np.ascontiguousarray(TEX["ab"])
    assert np.isfinite(ab).all() and (ab[:, 0] > 0).all()
    d, h = outs(len(ab))
    assert dev.dd_tex_pow(P(ab, f), P(d, f), P(h, f), len(ab)) == 0
    check("fmPow", d, TEX["pow"], ab)
    check("fmPow, host pass", h, TEX["pow"], ab)
    check("fmPow, device vs host pass", d, h, ab)


@pytest.mark.parametrize("cs,gamma", [(1, 2.2), (2, 1.0), (3, 1.0), (4, 1.0)])
def test_color_space_from_linear(dev, cs, gamma):
    rgb = np.ascontiguousarray(TEX["rgb"])
    d, h = np.empty_like(rgb), np.empty_like(rgb)
    assert dev.dd_tex_color_space(cs, f(gamma), P(rgb, f), P(d, f), P(h, f), len(rgb)) == 0
    check(f"colorSpaceFromLinear {cs}", d, TEX[f"cs1_{cs}"], rgb)
    check(f"colorSpaceFromLinear {cs}, host pass", h, TEX[f"cs1_{cs}"], rgb)
    check(f"colorSpaceFromLinear {cs}, device vs host pass", d, h, rgb)


def test_hsv_adjust(dev):
    rgb, sh = np.ascontiguousarray(TEX["rgb"]), np.ascontiguousarray(TEX["sat_hue"])
    d, h = np.empty_like(rgb), np.empty_like(rgb)
    assert dev.dd_tex_hsv(P(rgb, f), P(sh, f), P(d, f), P(h, f), len(rgb)) == 0
    check("rgbToHsv / hsvToRgb", d, TEX["hsv"], rgb, sh)
    check("rgbToHsv / hsvToRgb, host pass", h, TEX["hsv"], rgb, sh)
    check("rgbToHsv / hsvToRgb, device vs host pass", d, h, rgb, sh)


def test_cubic_interp(dev):
    cub = np.ascontiguousarray(TEX["cub"])
    d, h = (np.empty((len(cub), 4), np.float32) for _ in range(2))
    assert dev.dd_tex_cubic(P(cub, f), P(d, f), P(h, f), len(cub)) == 0
    check("cubicInterp", d, TEX["cubic"], cub)
    check("cubicInterp, host pass", h, TEX["cubic"], cub)
    check("cubicInterp, device vs host pass", d, h, cub)


BLEND_MODES = ["mix", "add", "mult", "sub", "screen", "div", "diff", "dark", "light", "overlay"]   # devscene.h BLEND_*


@pytest.mark.parametrize("mode", range(len(BLEND_MODES)), ids=BLEND_MODES)
def test_layer_blends_device_vs_host_pass(dev, mode):
    """blendRgb / blendValue have no golden vectors: the device against the host pass of the same source, on random
    (tex, out, fact, facg) in [-0.25, 1.25] and on the tuples that put a zero of either sign into divide's denominator."""
    rng = np.random.default_rng(40 + mode)
    n = 4096
    tex, out = (rng.uniform(-0.25, 1.25, (n, 3)).astype(np.float32) for _ in range(2))
    fact, facg = (rng.uniform(-0.25, 1.25, n).astype(np.float32) for _ in range(2))
    zt = rng.uniform(-0.25, 1.25, (64, 3)).astype(np.float32)
    for i in range(64):
        channels = i % 7 + 1                                  # every non-empty subset of the three channels
        zt[i, [k for k in range(3) if channels >> k & 1]] = -0.0 if i >= 32 else 0.0
    zo = rng.uniform(-0.25, 1.25, (64, 3)).astype(np.float32)
    zo[::4] = 0.0
    tex, out = np.ascontiguousarray(np.concatenate([tex, zt])), np.ascontiguousarray(np.concatenate([out, zo]))
    fact = L.f32(np.concatenate([fact, rng.uniform(-0.25, 1.25, 60), [0.0, 1.0, 0.0, 1.0]]))
    facg = L.f32(np.concatenate([facg, rng.uniform(-0.25, 1.25, 60), [0.0, 0.0, 1.0, 1.0]]))
    n = len(fact)
    d_rgb, h_rgb = (np.empty((n, 3), np.float32) for _ in range(2))
    d_val, h_val = outs(n)
    assert dev.dd_tex_blend(mode, P(tex, f), P(out, f), P(fact, f), P(facg, f), P(d_rgb, f), P(d_val, f), P(h_rgb, f), P(h_val, f), n) == 0
    check("blendRgb " + BLEND_MODES[mode], d_rgb, h_rgb, tex, out, fact, facg)
    check("blendValue " + BLEND_MODES[mode], d_val, h_val, tex, out, fact, facg)
