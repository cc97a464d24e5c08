"""Inputs and loaders shared by tests/test_devmath.py (devmath.h built by g++ for the host) and
tests/test_devmath_gpu.py (devmath.h and texeval.h built for gfx950): the g++ harness, the distributions of
tests/devmath_check.cc as numpy arrays, the libm input recipe, and the near-midpoint inputs that the host finds by
scanning whole binades."""
import ctypes as C
import functools
import os
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# index of a long double constant in both harnesses (devmath_host.cc kConsts, devmath_dev.hip constOf)
K_PI, K_DIV_PI_BY_2, K_DIV_1_BY_PI, K_MULT_PI_BY_2, K_DIV_1_BY_2PI, K_DIV_4_BY_PI, K_DIV_4_BY_SQUARED_PI = range(7)
# dm_scan_binade's `which`
SCAN_MUL, SCAN_MUL2_ABS, SCAN_MUL2, SCAN_MUL3, SCAN_MULDIV, SCAN_RECIP = range(6)

F = C.POINTER(C.c_float)
U = C.POINTER(C.c_uint32)


def P(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def f32(a):
    return np.ascontiguousarray(a, np.float32)


def same_bits(a, b):
    """Element-wise: the same bit pattern, or a NaN on both sides."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (a.dtype, b.dtype, a.shape, b.shape)
    if a.dtype.kind != "f":
        return a == b
    u = np.uint32 if a.dtype == np.float32 else np.uint64
    return (a.view(u) == b.view(u)) | (np.isnan(a) & np.isnan(b))


def describe(name, ok, got, want, *inputs):
    """An assertion message with the first mismatching inputs and both bit patterns."""
    bad = np.flatnonzero(~ok.reshape(len(ok), -1).all(1))[:3]
    rows = []
    for i in bad:
        ins = ", ".join(repr(np.asarray(a[i]).tolist()) for a in inputs)
        rows.append(f"input ({ins}): got {np.atleast_1d(got[i]).view(_uint(got)).tolist()} want {np.atleast_1d(want[i]).view(_uint(want)).tolist()}")
    return f"{name}: {int((~ok).sum())} of {ok.size} values differ; " + "; ".join(rows)


def _uint(a):
    return {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]


@functools.lru_cache(maxsize=None)
def host_lib():
    """tests/devmath_host.cc built as tests/test_devmath.py builds it."""
    out = os.path.join(tempfile.mkdtemp(prefix="yaf_devmath_"), "devmath_host.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-shared", "-fPIC", "-o", out,
                    os.path.join(HERE, "devmath_host.cc")], check=True)
    return C.CDLL(out)


# ---- the distributions of tests/devmath_check.cc ----
N_X87 = 1_000_000


@functools.lru_cache(maxsize=None)
def x87_inputs():
    """x: U(-30, 30), every 7th in [0, 7), every 11th a random significand and sign at a binary exponent in [-27, 12];
    a, b: U(1e-4, 50); pr: (float)paths * radius^2 of the photon density scale; s2: U[0, 1)."""
    rng = np.random.default_rng(12345)
    n = N_X87
    x = rng.uniform(-30, 30, n).astype(np.float32)
    x[::7] = (rng.random(len(x[::7]), dtype=np.float32) * np.float32(7))
    bits = rng.integers(0, 2 ** 32, len(x[::11]), dtype=np.uint64).astype(np.uint32)
    expo = (rng.integers(0, 40, len(bits)) + 100).astype(np.uint32)
    x[::11] = ((bits & np.uint32(0x807fffff)) | (expo << np.uint32(23))).view(np.float32)
    a = rng.uniform(1e-4, 50, n).astype(np.float32)
    b = rng.uniform(1e-4, 50, n).astype(np.float32)
    pr = (1 + rng.integers(0, 20_000_000, n)).astype(np.float32) * (a * np.float32(1e-3))
    s2 = rng.random(n, dtype=np.float32)
    out = dict(x=x, a=a, b=b, pr=pr, s2=s2)
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def sphere_inputs():
    """The acos values of test_sphere_v_long_double: the 1,000,001-point grid of [0, pi], random floats, the edges."""
    rng = np.random.default_rng(12)
    a = np.concatenate([np.linspace(0, np.pi, 1_000_001, dtype=np.float32), rng.uniform(0, np.pi, 1_000_000).astype(np.float32),
                        np.float32([0.0, np.float32(np.pi), np.float32(np.pi / 2)])])
    a = f32(a)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def kernel_inputs():
    """(x, y, z) of the photon kernel 3 ir2 / pi (1 - d2 ir2)^2 (sample.h:31-35) as k_gather draws them (a gather radius,
    a photon inside it), then uniform positives."""
    rng = np.random.default_rng(31)
    n = N_X87 // 2
    r = rng.uniform(0.01, 2.0, n).astype(np.float32)
    r2 = r * r
    ir2 = np.float32(1) / r2
    d2 = rng.random(n, dtype=np.float32) * r2
    sk = np.maximum(np.float32(1) - d2 * ir2, np.float32(0))
    pos = rng.uniform(1e-4, 50, (3, n)).astype(np.float32)
    x = f32(np.concatenate([np.float32(3) * ir2, pos[0]]))
    y = f32(np.concatenate([sk, pos[1]]))
    z = f32(np.concatenate([sk, pos[2]]))
    for v in (x, y, z):
        v.setflags(write=False)
    return x, y, z


@functools.lru_cache(maxsize=None)
def round_inputs():
    """Double-doubles (hi, lo) with hi > 0 and |lo| <= ulp(hi) / 2 for round64 and round24, made so that every case of
    the two roundings occurs thousands of times, the ties included, which the x87 products reach for about one input
    in 2^40: hi = (I + frac) 2^(e - 23) with I a 24-bit integer and frac one of 0, 1/2 (a float midpoint) or 29 random
    bits; lo = t 2^(e - 63), t in units of the 64-bit significand's last place: 0, an integer, a half-integer (a tie of
    the first rounding), a half-integer +- 2^-30, or any double in (-1023, 1023); and hi a power of two with lo < 0."""
    rng = np.random.default_rng(64)
    n = 240_000
    e = rng.integers(-60, 61, n)
    big = rng.integers(2 ** 23, 2 ** 24, n).astype(np.float64)
    fk = rng.integers(0, 4, n)
    frac = np.where(fk == 0, 0.0, np.where(fk <= 2, 0.5, rng.integers(0, 2 ** 29, n) / 2.0 ** 29))
    k = rng.integers(-1023, 1023, n).astype(np.float64)
    tk = rng.integers(0, 5, n)
    t = np.select([tk == 0, tk == 1, tk == 2, tk == 3], [0.0 * k, k, k + 0.5, k + 0.5 + rng.choice([-1.0, 1.0], n) * 2.0 ** -30],
                  rng.uniform(-1023, 1023, n))
    pow2 = rng.random(n) < 0.05
    big = np.where(pow2, 2.0 ** 23, big)
    frac = np.where(pow2, 0.0, frac)
    t = np.where(pow2, -np.abs(t) / 2, t)
    hi = np.ascontiguousarray(np.ldexp(big + frac, e - 23))
    lo = np.ascontiguousarray(np.ldexp(t, e - 63))
    assert (hi + lo == hi).all()
    hi.setflags(write=False)
    lo.setflags(write=False)
    return hi, lo


# ---- near-midpoint inputs: the slow branch of every dispatcher ----
# (dispatcher, which, constant, [(biased exponent of x, y, z)]): at least four binades each; safeToRound rejects about
# 2e-6 of inputs, so about 17 per binade
SCANS = {
    "x87mul": [(SCAN_MUL, c, [(e, 0.0, 0.0) for e in (122, 125, 127, 130)])
               for c in (K_DIV_4_BY_PI, K_MULT_PI_BY_2, K_DIV_1_BY_PI)],
    "x87mul2": [(SCAN_MUL2_ABS, K_DIV_4_BY_SQUARED_PI, [(e, 0.0, 0.0) for e in (121, 123, 125, 126, 127, 128)]),
                (SCAN_MUL2, K_DIV_4_BY_SQUARED_PI, [(124, 0.7321, 0.0), (129, 17.25, 0.0)])],
    "x87mul3": [(SCAN_MUL3, K_DIV_1_BY_PI, [(126, 0.3712, 0.3712), (128, 0.8125, 0.8125), (131, 0.05127, 0.05127),
                                            (134, 0.9931, 0.9931), (127, 3.25, 11.7), (137, 0.6021, 0.6021)])],
    "x87mulDiv": [(SCAN_MULDIV, K_PI, [(124, 0.7321, 0.0), (127, 3.117, 0.0), (130, 41.03, 0.0)]),
                  (SCAN_MULDIV, K_MULT_PI_BY_2, [(119, 0.01173, 0.0), (126, 1.0, 0.0), (128, 5.5, 0.0)])],
    "x87recipMul": [(SCAN_RECIP, K_PI, [(e, 0.0, 0.0) for e in (117, 124, 127, 133, 140, 146)])],
}
NEAR_MIN = 50


@functools.lru_cache(maxsize=None)
def near_midpoint(dispatcher):
    """[(constant, x, y, z)] arrays of the inputs of the scanned binades for which safeToRound is false, per scan of the
    dispatcher, found by the g++ harness on the CPU; and their total count."""
    lib = host_lib()
    lib.dm_scan_binade.restype = C.c_int
    cap = 4096
    out, total = [], 0
    for which, c, binades in SCANS[dispatcher]:
        xs, ys, zs = [], [], []
        for expo, y, z in binades:
            buf = np.empty(cap, np.float32)
            n = lib.dm_scan_binade(which, c, expo, C.c_float(y), C.c_float(z), P(buf, C.c_float), cap)
            assert 0 <= n <= cap, (dispatcher, expo, n)
            x = buf[:n]
            xs.append(x)
            ys.append(np.abs(x) if which == SCAN_MUL2_ABS else np.full(n, y, np.float32))
            zs.append(np.full(n, z, np.float32))
        x, y, z = (f32(np.concatenate(v)) for v in (xs, ys, zs))
        total += len(x)
        out.append((c, x, y, z))
    return out, total


# ---- libm restatements ----
LIBM_NAMES = ("atan2f", "acosf", "asinf", "atanf", "mathAsin")


@functools.lru_cache(maxsize=None)
def libm_inputs():
    """(y, x): the 2.4 M inputs of test_libm_restatements_match_host_libm (uniform in [-1, 1]^2, random exponents, raw
    bit patterns), then the edges by name: +-0, +-inf, NaN, subnormals, the branch thresholds of the fdlibm code."""
    rng = np.random.default_rng(11)
    n = 800_000
    parts = []
    for _ in range(2):
        parts.append([rng.uniform(-1, 1, n).astype(np.float32),
                      (rng.uniform(-1, 1, n) * 2.0 ** rng.integers(-30, 30, n)).astype(np.float32),
                      rng.integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    edge_bits = [0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x23000000, 0x23000001, 0x31000000, 0x30ffffff, 0x32000000,
                 0x31ffffff, 0x3ee00000, 0x3edfffff, 0x3f000000, 0x3effffff, 0x3f300000, 0x3f79999a, 0x3f799999, 0x3f7fffff,
                 0x3f800000, 0x3f800001, 0x3f980000, 0x401c0000, 0x4bffffff, 0x4c000000, 0x7f7fffff, 0x7f800000, 0x7fc00000]
    edges = np.array(edge_bits + [b | 0x80000000 for b in edge_bits], np.uint32).view(np.float32)
    ey, ex = np.meshgrid(edges, edges, indexing="ij")
    y = f32(np.concatenate(parts[0] + [ey.ravel()]))
    x = f32(np.concatenate(parts[1] + [ex.ravel()]))
    y.setflags(write=False)
    x.setflags(write=False)
    return y, x


def host_libm(lib):
    """{name: (restatement, libm)} on libm_inputs() from the g++ harness."""
    y, x = libm_inputs()
    dev = [np.empty(len(y), np.float32) for _ in LIBM_NAMES]
    ref = [np.empty(len(y), np.float32) for _ in LIBM_NAMES]
    lib.dm_libm_all(P(y, C.c_float), P(x, C.c_float), len(y), (F * 5)(*[P(o, C.c_float) for o in dev]),
                    (F * 5)(*[P(o, C.c_float) for o in ref]))
    return {k: (d, r) for k, d, r in zip(LIBM_NAMES, dev, ref)}


# ---- Halton ----
HALTON_K = 16


def halton(fn, base, starts, k=HALTON_K):
    """(status, first [n], next [n, k], inc [n, k]) of dm_halton / dd_halton."""
    starts = np.ascontiguousarray(starts, np.uint32)
    n = len(starts)
    first = np.empty(n, np.float32)
    nxt = np.empty((n, k), np.float32)
    inc = np.full((n, k), np.nan, np.float32)
    st = fn(C.c_uint32(int(base)), P(starts, C.c_uint32), n, k, P(first, C.c_float), P(nxt, C.c_float), P(inc, C.c_float))
    return st, first, nxt, inc


def faure_perm(b):
    """render.cc faurePerm, as test_low_discrepancy_faure rebuilds it."""
    if b <= 2:
        return [0, 1]
    if b % 2 == 0:
        h = faure_perm(b // 2)
        return [2 * v for v in h] + [2 * v + 1 for v in h]
    p, c = faure_perm(b - 1), (b - 1) // 2
    out = []
    for i, v in enumerate(p):
        if i == c:
            out.append(c)
        out.append(v + (v >= c))
    return out


def primes_table():
    primes = [1]
    c = 2
    while len(primes) < 50:
        if all(c % q for q in range(2, int(c ** 0.5) + 1)):
            primes.append(c)
        c += 1
    return primes


def udiv_cases():
    """(d, numerators) of test_magic_division_exact."""
    rng = np.random.default_rng(7)
    n = np.concatenate([np.arange(0, 5000), 2**32 - 1 - np.arange(0, 5000), rng.integers(0, 2**32, 200000)]).astype(np.uint32)
    primes = [p for p in range(2, 260) if all(p % q for q in range(2, int(p**0.5) + 1))]
    for d in primes + [2**31, 2**31 - 1, 1000003]:
        nn = np.concatenate([n, (np.arange(1, 4000, dtype=np.uint64) * d % 2**32).astype(np.uint32)])
        yield d, np.ascontiguousarray(np.concatenate([nn, nn - 1, nn + 1]).astype(np.uint32))
