"""Pin the CPU oracle (oracle/yafcpu.cc) against the reference's own code:
(1) the committed golden vectors of tests/golden/prims.npz, prims_r02.npz and prims_filters.npz (made by
    make_golden_prims.py from oracle/_ref, i.e. the reference sources compiled here), always;
(2) the live reference building blocks on fresh random inputs, when oracle/_ref is built."""
import os
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
G = np.load(os.path.join(HERE, "golden", "prims.npz"))


@pytest.fixture(scope="module")
def o(oracle_built):
    return oracle_built.oracle_prims()


def same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.dtype.kind == "f":
        return np.array_equal(a.view(np.uint32 if a.dtype == np.float32 else np.uint64),
                              b.astype(a.dtype).view(np.uint32 if a.dtype == np.float32 else np.uint64))
    return np.array_equal(a, b)


@pytest.mark.parametrize("w", ["riVdC", "riS", "riLp"])
def test_radical_inverse(o, w):
    assert same(o.ri(w, G["ri_bits"], G["ri_r"]), G[w])


def test_fnv(o):
    assert same(o.fnv32(G["fnv_in"]), G["fnv"])


def test_low_discrepancy_faure(o):
    assert same(o.lds(G["lds_dim"], G["lds_idx"]), G["lds"])


def test_halton_incremental(o):
    for base, start, seq in zip(G["halton_bases"], G["halton_starts"], G["halton_seq"]):
        assert same(o.halton_seq(int(base), int(start), len(seq)), seq), (base, start)


def test_fast_trig_and_exp(o):
    assert same(o.unary("sin", G["trig_x"]), G["sin"])
    assert same(o.unary("cos", G["trig_x"]), G["cos"])
    assert same(o.unary("exp", G["exp_x"]), G["exp"])


def test_vectors_and_hemisphere(o):
    assert same(o.unary("coords_system", G["coords_in"].reshape(-1), 6, 3).reshape(-1, 6), G["coords"])
    assert same(o.unary("normalize", G["norm_in"].reshape(-1), 3, 3).reshape(-1, 3), G["norm"])
    assert same(o.cos_hemisphere(G["hemi_nrv"], G["hemi_s"]), G["hemi"])


def test_bound_cross(o):
    assert same(o.bound_cross(G["bound_box"], G["bound_ray"]), G["bound"])


def test_mwc(o):
    for seed, ref in zip(G["mwc_seeds"], G["mwc"]):
        assert same(o.mwc(int(seed), len(ref)), ref)


def test_film_filter_and_rounding(o):
    assert same(o.unary("filter_gauss", G["gauss_in"].reshape(-1), 1, 2), G["gauss"])
    assert same(o.int_of_double("round_to_int", G["int_in"]), G["round_to_int"])
    assert same(o.int_of_double("floor_to_int", G["int_in"]), G["floor_to_int"])
    assert same(o.clamp_proportional(G["clamp_in"], 1.5), G["clamp_1_5"])
    assert same(o.clamp_proportional(G["clamp_in"], 0.0), G["clamp_0"])


def test_live_reference_random_inputs(o, oracle_built):
    r = oracle_built.ref_prims()
    if r is None:
        pytest.skip("oracle/_ref not built (reference tree absent): golden vectors above still pin the oracle")
    rng = np.random.default_rng(99)
    n = 100000
    b = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    rr = rng.integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
    for w in ("riVdC", "riS", "riLp"):
        assert same(o.ri(w, b, rr), r.ri(w, b, rr))
    dims = rng.integers(1, 50, n).astype(np.int32)
    assert same(o.lds(dims, b), r.lds(dims, b))
    x = rng.uniform(-50, 50, n).astype(np.float32)
    assert same(o.unary("sin", x), r.unary("sin", x))
    assert same(o.unary("cos", x), r.unary("cos", x))


# ---- round 2 (tests/golden/prims_r02.npz): src/geometry/vector.cc shirleyDisk, src/color/color.cc +
# color.h Rgbe, src/render/imagesplitter.cc tile lists ----
G2 = np.load(os.path.join(HERE, "golden", "prims_r02.npz"))


def test_shirley_disk(o):
    assert same(o.shirley(G2["shirley_in"]), G2["shirley"])


def test_rgbe_decode(o):
    assert same(o.rgbe(G2["rgbe_in"]), G2["rgbe"])


def _centre_key(t, w, h):
    return (t[:, 0] - w // 2) ** 2 + (t[:, 1] - h // 2) ** 2


@pytest.mark.parametrize("k", range(6))
def test_tile_lists(o, k):
    w, h, bs = (int(v) for v in G2["tiles_sizes"][k])
    lin = G2[f"tiles_linear_{k}"]
    assert np.array_equal(o.tiles(w, h, bs, "linear"), lin)
    # centre: the reference shuffles with std::random_device before its (unstable) sort, so only the
    # key sequence is determined; the oracle / GPU keep linear order among ties (one of its outcomes)
    ref_c, ours = G2[f"tiles_centre_{k}"], o.tiles(w, h, bs, "centre")
    assert np.array_equal(np.sort(ref_c.view([("", ref_c.dtype)] * 4), axis=0), np.sort(ours.view([("", ours.dtype)] * 4), axis=0))
    assert np.array_equal(_centre_key(ref_c, w, h), _centre_key(ours, w, h))
    kk = _centre_key(ours, w, h)
    assert np.all(np.diff(kk) >= 0)
    # the reference with 8 render threads subdivides its last 16 tiles; the GPU and the oracle
    # render the one-thread list (documented): the lists agree up to there
    t8 = G2[f"tiles_linear_t8_{k}"]
    m = max(0, len(lin) - 16)
    assert np.array_equal(t8[:m], lin[:m])


def test_live_reference_round2_random_inputs(o, oracle_built):
    r = oracle_built.ref_prims()
    if r is None:
        pytest.skip("oracle/_ref not built (reference tree absent): golden vectors above still pin the oracle")
    rng = np.random.default_rng(7)
    r12 = rng.random((50000, 2)).astype(np.float32)
    assert same(o.shirley(r12), r.shirley(r12))
    b = rng.integers(0, 256, (50000, 4), dtype=np.uint8)
    assert same(o.rgbe(b), r.rgbe(b))
    for w, h, bs in [(37, 29, 5), (640, 480, 32), (1, 1, 16)]:
        assert np.array_equal(o.tiles(w, h, bs, "linear"), r.tiles(w, h, bs, "linear"))


# ---- film filter functions (tests/golden/prims_filters.npz: include/math/filter.h mitchell, lanczos2 at the film
# table's 256 points, (0, 0), the float neighbourhoods of r = 0.5 and r = 1, and 10^5 points of [0, 1.5)^2) ----
GF = np.load(os.path.join(HERE, "golden", "prims_filters.npz"))


def filter_random_points():
    """The fixture's random inputs, regenerated (integer arithmetic) and checked against its checksum."""
    sys.path.insert(0, os.path.join(HERE, "golden"))
    import make_golden_prims as M
    rnd = M.splitmix_points(int(GF["random_n"][0]), int(GF["random_seed"][0]))
    assert np.array_equal(M.points_checksum(rnd), GF["random_checksum"]) and same(rnd[:16], GF["random_head"])
    assert len(rnd) == 100000 and rnd.min() >= 0 and rnd.max() < 1.5
    return rnd


def test_filter_fixture_covers_the_branches():
    p = GF["points"].astype(np.float64)
    r = np.hypot(p[:, 0], p[:, 1])
    assert len(p) >= 256 + 1 + 100 and (p == 0).all(1).any()
    for edge in (0.5, 1.0):
        near = np.abs(r - edge) < 1e-6
        assert (r[near] < edge).any() and (r[near] > edge).any()
    assert (GF["mitchell"] < 0).any() and (GF["lanczos"] < 0).any()      # signed lobes
    assert (GF["mitchell_random"] < 0).sum() > 1000 and (GF["lanczos_random"] < 0).sum() > 1000


@pytest.mark.parametrize("name", ["mitchell", "lanczos"])
def test_film_filter_signed(o, name):
    assert same(o.film_filter(name, GF["points"]), GF[name])
    assert same(o.film_filter(name, filter_random_points()), GF[name + "_random"])


def test_live_reference_film_filters_random_inputs(o, oracle_built):
    r = oracle_built.ref_prims()
    if r is None:
        pytest.skip("oracle/_ref not built (reference tree absent): golden vectors above still pin the oracle")
    rng = np.random.default_rng(4242)
    d = np.concatenate([rng.uniform(-1.5, 1.5, (100000, 2)), rng.uniform(-0.01, 0.01, (1000, 2)),
                        rng.uniform(-2.5, 2.5, (10000, 2))]).astype(np.float32)
    assert same(o.film_filter("gauss", d), r.film_filter("gauss", d))
    if not (r.has("filter_mitchell") and r.has("filter_lanczos2")):
        # an oracle/_ref kept from before ref_harness.cc had these two (make ref rebuilds it only where the
        # reference tree is present)
        pytest.skip("oracle/_ref predates ref_filter_mitchell / ref_filter_lanczos2 and was not rebuilt (reference tree "
                    "absent): gauss checked; golden vectors above still pin mitchell and lanczos")
    for name in ("mitchell", "lanczos"):
        assert same(o.film_filter(name, d), r.film_filter(name, d)), name


# ---- the colour arithmetic under ImageFilm::nextPass (tests/golden/prims_aa.npz: color.h colorDifference with and
# without the r, g, b, a components, normalized, abscol2Bri; negative, zero and subnormal weights, negative
# components, inf and NaN among the inputs) ----
GA = np.load(os.path.join(HERE, "golden", "prims_aa.npz"))


def test_aa_fixture_covers_the_special_values():
    w = GA["cw"][:, 4]
    tiny = np.finfo(np.float32).tiny
    assert (w == 0).any() and (w < 0).any() and ((np.abs(w) > 0) & (np.abs(w) < tiny)).any()
    for a in (GA["pairs"], GA["cw"][:, :4], GA["rgb"]):
        assert (a < 0).any() and np.isinf(a).any() and np.isnan(a).any()
    # a zero weight gives the zero colour, a negative one divides (color.h:554-558)
    assert (GA["normalized"][w == 0] == 0).all()
    neg = (w < -1e-3) & (w > -1e3) & (np.abs(GA["cw"][:, 0]) > 1e-3) & (np.abs(GA["cw"][:, 0]) < 1e3)
    assert neg.any() and (np.sign(GA["normalized"][neg, 0]) == -np.sign(GA["cw"][neg, 0])).all()
    # the r, g, b, a components only ever raise the difference, and alpha alone can
    assert (GA["color_difference_rgb"] > GA["color_difference_bri"]).any()


def test_aa_colour_arithmetic(o):
    assert same(o.color_difference(GA["pairs"], False), GA["color_difference_bri"])
    assert same(o.color_difference(GA["pairs"], True), GA["color_difference_rgb"])
    assert same(o.normalized(GA["cw"]), GA["normalized"])
    assert same(o.abscol2bri(GA["rgb"]), GA["abscol2bri"])


def test_live_reference_aa_colour_arithmetic_random_inputs(o, oracle_built):
    r = oracle_built.ref_prims()
    if r is None:
        pytest.skip("oracle/_ref not built (reference tree absent): golden vectors above still pin the oracle")
    if not (r.has("color_difference") and r.has("normalized") and r.has("abscol2bri")):
        pytest.skip("oracle/_ref predates ref_color_difference / ref_normalized / ref_abscol2bri and was not rebuilt "
                    "(reference tree absent): golden vectors above still pin the oracle")
    rng = np.random.default_rng(777)
    pairs = np.concatenate([rng.normal(0, 2, (100000, 8)), rng.integers(-16, 33, (20000, 8)) / 8.0]).astype(np.float32)
    cw = rng.normal(0, 2, (100000, 5)).astype(np.float32)
    cw[::7, 4] = 0
    for flag in (False, True):
        assert same(o.color_difference(pairs, flag), r.color_difference(pairs, flag)), flag
    assert same(o.normalized(cw), r.normalized(cw))
    assert same(o.abscol2bri(pairs[:, :3]), r.abscol2bri(pairs[:, :3]))


# the table of ImageFilm::darkThresholdCurveInterpolate (imagefilm.cc:799-815, not linkable on its own): segment
# ends (brightness, threshold); constant below the first and above the last
DARK_CURVE = [(0.10, 0.0001), (0.20, 0.0010), (0.30, 0.0020), (0.40, 0.0035), (0.50, 0.0055), (0.60, 0.0075), (0.70, 0.0100),
              (0.80, 0.0150), (0.90, 0.0250), (1.00, 0.0400), (1.20, 0.0800), (1.40, 0.0950), (1.80, 0.1000)]


def dark_curve_table(b):
    """The curve from the table, in the reference's float32 expression order: lo + (b - b_lo) * (hi - lo) / (b_hi - b_lo)."""
    f = np.float32
    b = f(b)
    if b <= f(DARK_CURVE[0][0]):
        return f(DARK_CURVE[0][1])
    for (b0, t0), (b1, t1) in zip(DARK_CURVE[:-1], DARK_CURVE[1:]):
        if b <= f(b1):
            width = f(round(b1 - b0, 2))     # the reference writes the segment widths as the literals 0.10f, 0.20f, 0.40f
            return f(f(t0) + f(f(f(b - f(b0)) * f(f(t1) - f(t0))) / width))
    return f(DARK_CURVE[-1][1])


def test_dark_threshold_curve_table(oracle_built):
    """The oracle's curve at, just below and just above each breakpoint (and at 0, far above and negative)."""
    f = np.float32
    pts = [f(0.0), f(-1.0), f(5.0), f(np.inf)]
    for b, _ in DARK_CURVE:
        pts += [np.nextafter(f(b), f(-np.inf)), f(b), np.nextafter(f(b), f(np.inf))]
    pts += [f(0.15), f(0.55), f(1.1), f(1.6)]
    pts = np.array(pts, f)
    got = oracle_built.dark_threshold_curve(pts)
    want = np.array([dark_curve_table(b) for b in pts], f)
    assert same(got, want), [(float(b), float(g), float(w)) for b, g, w in zip(pts, got, want) if g != w]
    # the curve is continuous to float rounding and never decreases
    order = np.argsort(pts[np.isfinite(pts)])
    assert (np.diff(got[np.isfinite(pts)][order]) >= -1e-9).all()


# ---- texturing building blocks (tests/golden/tex_prims.npz, made by make_golden_tex.py from the
# reference's own image_buffers.h / color.h / interpolation.h / math.h) ----
TEX_KINDS = {0: "Rgba1010108", 1: "Rgb101010", 2: "Rgba7773", 3: "Rgb565", 4: "Gray8", 5: "Gray", 6: "GrayAlpha", 7: "RgbAlpha"}


@pytest.fixture(scope="module")
def tex_golden():
    return np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tex_prims.npz"))


def test_oracle_texturing_primitives_bitexact(oracle_built, tex_golden):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
    import make_golden_tex as M
    g = tex_golden
    got = M.run(oracle_built.oracle_lib(), "yc_", g["rgba"], g["rgb"], g["sat_hue"], g["cub"], g["ab"])
    for k, v in got.items():
        assert np.array_equal(v.view(np.uint32), g[k].view(np.uint32)), f"{k}: {(v.view(np.uint32) != g[k].view(np.uint32)).sum()} mismatches"


def test_product_image_buffers_quantise_like_the_reference(product, tex_golden):
    """yafaray_createImage + setImageColor / getImageColor through every buffer type (host code of
    the drop-in library: no GPU involved) against the reference's own buffer classes."""
    kinds = {0: ("ColorAlpha", "optimized"), 1: ("Color", "optimized"), 2: ("ColorAlpha", "compressed"),
             3: ("Color", "compressed"), 4: ("Gray", "optimized"), 5: ("Gray", "none"), 6: ("GrayAlpha", "none"),
             7: ("ColorAlpha", "none")}
    rgba = tex_golden["rgba"][:1024]
    yi = product.Interface()
    yi.createScene()
    for kind, (typ, opt) in kinds.items():
        yi.paramsClearAll()
        yi.paramsSetString("type", typ)
        yi.paramsSetString("image_optimization", opt)
        yi.paramsSetInt("width", 32)
        yi.paramsSetInt("height", 32)
        h = yi.createImage(f"img{kind}")
        assert h, typ + "/" + opt
        out = np.empty_like(rgba)
        for i, c in enumerate(rgba):
            yi.setImageColor(h, i % 32, i // 32, *map(float, c))
            out[i] = yi.getImageColor(h, i % 32, i // 32)
        ref = tex_golden[f"quant{kind}"][:1024]
        assert np.array_equal(out.view(np.uint32), ref.view(np.uint32)), f"{TEX_KINDS[kind]}: {(out != ref).sum()} mismatches"
    yi.close()


@pytest.mark.parametrize("seed", [1, 2, 7920, 0x7fffffff, 0])
def test_glibc_rand_restatement(oracle_built, seed):
    """The oracle seeds each tile's Russian-roulette generator from a restatement of glibc's rand()
    (integrator_tiled.cc:272, the reference's scene setup reseeds with srand); pinned here against
    the real libc: srand(seed) then 2000 rand() calls (seed 0 behaves as seed 1 in glibc)."""
    import ctypes as C
    libc = C.CDLL("libc.so.6")
    libc.srand.argtypes = [C.c_uint]
    libc.rand.restype = C.c_int
    n = 2000
    libc.srand(seed)
    want = np.array([libc.rand() for _ in range(n)], np.uint32)
    got = oracle_built.glibc_rand(seed, n)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:5]
