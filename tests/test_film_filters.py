"""Wide and signed film filters against the oracle, bit for bit.

k_film (and k_layer_film) has a static 2x2 form for footprints that reach one pixel forward and none back, and a
generic run-time window (<= 9x9, the sources insertion-sorted by splat rank) for every other filter.  The scenes here
have exact samples (filmlib.exact_scene: three emitters, no lights), k_film sums a pixel's sources in the
reference's one-thread splat order without contraction, so the product's film must equal the oracle's bitwise,
colours and weights: no ULP tolerance anywhere in this file.  Every case first requires that of the same spec
under box 1.0 (the narrowest footprint: a sample's own pixel, and the next one only from dx or dy >= 0.999), so a
shading difference is not mistaken for a film one.

The filter matrix, with the film set-up the product's host code computes (hm::filmSetup; pinned below against
the oracle's FilmTable and against the footprint formula of imagefilm.cc:684-687):

    filter    AA_pixelwidth  filterw          reach fwd/back  kernel form
    box       3.0            1.5              1/1             generic
    gauss     4.0            4.0 (clamped)    4/3             generic, 8x8 window
    mitchell  1.0            1.3              1/0             static, signed table
    mitchell  1.5            1.95             2/1             generic
    mitchell  4.0            4.0 (clamped)    4/3             generic, 8x8 window
    lanczos   1.0            0.501 (clamped)  1/0             static
    lanczos   2.0            1.0              1/0             static, signed table
    lanczos   3.0            1.5              1/1             generic
    lanczos   5.0            2.5              2/2             generic
    lanczos   7.0            3.5              3/3             generic
    lanczos   8.0            4.0              4/3             generic, 8x8 window

(at the half-integers roundToInt's truncation of v + 0.5 - 1.4e-11 decides the reach.)
"""
import numpy as np
import pytest

import filmlib as FL
from filmlib import bits
from libyafaray_amd import scenes

# (filter, AA_pixelwidth): (filterw, reach forward, reach back) by hand
MATRIX = {("box", 3.0): (1.5, 1, 1), ("gauss", 4.0): (4.0, 4, 3), ("mitchell", 1.0): (1.3, 1, 0),
          ("mitchell", 1.5): (1.95, 2, 1), ("mitchell", 4.0): (4.0, 4, 3), ("lanczos", 1.0): (0.501, 1, 0),
          ("lanczos", 2.0): (1.0, 1, 0), ("lanczos", 3.0): (1.5, 1, 1), ("lanczos", 5.0): (2.5, 2, 2),
          ("lanczos", 7.0): (3.5, 3, 3), ("lanczos", 8.0): (4.0, 4, 3)}
ALL = list(MATRIX)
WIDE = [("gauss", 4.0), ("mitchell", 4.0), ("lanczos", 8.0), ("mitchell", 1.0)]   # the 4/3 reaches + one signed static
PINNED_BEFORE = [("box", 1.0), ("gauss", 1.0), ("gauss", 1.5)]


def fid(f):
    return "%s%g" % f


# ---------------------------------------------------------------------------------------------------------------
# CPU: the product's host filter functions and film set-up
# ---------------------------------------------------------------------------------------------------------------
def test_host_filter_functions_match_the_reference_vectors():
    """hm::filterBox / Gauss / Mitchell / Lanczos (hostmath.h, the code that fills the product's table) against the
    reference's own outputs: tests/golden/prims.npz (gauss) and prims_filters.npz (mitchell, lanczos2)."""
    import test_oracle_golden as T      # the fixtures and the regenerated random inputs, as the oracle's pin uses them
    g, gf = T.G, T.GF
    assert np.array_equal(bits(FL.host_filter("gauss", g["gauss_in"])), bits(g["gauss"]))
    assert np.all(FL.host_filter("box", gf["points"]) == 1.0)
    rnd = T.filter_random_points()
    for name in ("mitchell", "lanczos"):
        assert np.array_equal(bits(FL.host_filter(name, gf["points"])), bits(gf[name])), name
        assert np.array_equal(bits(FL.host_filter(name, rnd)), bits(gf[name + "_random"])), name


@pytest.mark.parametrize("filt", ALL + PINNED_BEFORE, ids=fid)
def test_host_film_setup_equals_the_oracle_table(oracle_built, filt):
    su = FL.film_setup(*filt)
    tab, fw, ts = oracle_built.film_table(*filt)
    assert np.array_equal(bits(su.table), bits(tab))
    assert bits(np.float32(su.filterw)) == bits(np.float32(fw)) and bits(np.float32(su.table_scale)) == bits(np.float32(ts))
    # the reach from the footprint formula (imagefilm.cc:684-687) at the extreme sub-pixel positions
    below_one = float(np.nextafter(np.float32(1), np.float32(0)))
    f = float(np.float32(su.filterw))
    assert su.reach_fwd == max(0, FL._round_to_int(below_one + f - 1.0))
    assert su.reach_back == max(0, -FL._round_to_int(0.0 - f))
    if filt in MATRIX:
        hw, rf, rb = MATRIX[filt]
        # (the hand width is a decimal: 0.75f * 2.6f is one float below 1.95f; the bitwise pin is the oracle's above)
        assert abs(su.filterw - hw) < 1e-6 and (su.reach_fwd, su.reach_back) == (rf, rb)
    assert (su.table < 0).any() == (filt[0] in ("mitchell", "lanczos"))      # the signed tables


# ---------------------------------------------------------------------------------------------------------------
# the cases
# ---------------------------------------------------------------------------------------------------------------
def _crop(**kw):
    return FL.exact_scene(40, 30, 2, tile_size=5, **kw).with_render(width=13, height=9, xstart=11, ystart=6)


SHAPES = {
    "base": lambda **kw: FL.exact_scene(23, 17, 2, tile_size=5, **kw),                      # ragged tiles, window over 2-3 tiles
    "tile3-linear": lambda **kw: FL.exact_scene(23, 17, 2, tile_size=3, tiles_order="linear", **kw),
    "tile3-centre": lambda **kw: FL.exact_scene(23, 17, 2, tile_size=3, tiles_order="centre", **kw),
    "tile3-random": lambda **kw: FL.exact_scene(23, 17, 2, tile_size=3, tiles_order="random", **kw),
    "narrow": lambda **kw: FL.exact_scene(7, 5, 3, tile_size=32, **kw),                     # film narrower than the 8x8 window
    "2x2": lambda **kw: FL.exact_scene(2, 2, 1, tile_size=1, **kw),
    "1x1": lambda **kw: FL.exact_scene(1, 1, 1, tile_size=4, **kw),
    "crop": _crop,                                                                          # pixel hash in camera coordinates
    "clamp": lambda **kw: FL.exact_scene(23, 17, 2, tile_size=5, clamp_samples=1.0, **kw),  # clampProportionalRgb per splat
    "part-linear": lambda **kw: FL.exact_scene(23, 17, 1, tile_size=5, tiles_order="linear", **kw),
    "part-centre": lambda **kw: FL.exact_scene(23, 17, 1, tile_size=5, tiles_order="centre", **kw),
}
ADAPTIVE = dict(aa_passes=3, aa_inc_samples=2, aa_threshold=0.05)
SHAPES["adaptive"] = lambda **kw: FL.exact_scene(40, 30, 1, tile_size=7, **ADAPTIVE, **kw)
SHAPES["adaptive-curve"] = lambda **kw: FL.exact_scene(40, 30, 1, tile_size=7, aa_detect_color_noise=True,
                                                       aa_dark_detection_type="curve", **ADAPTIVE, **kw)
SHAPES["bands"] = lambda **kw: FL.exact_scene(23, 10, 2, tile_size=5, **kw)      # 3 members: bands of 3 or 4 rows < reach 4
SPP1 = ["2x2", "1x1", "part-linear", "part-centre"]                             # one pass, one sample: dx = dy = 0.5
PARTIAL_FILTERS = [("mitchell", 1.5), ("mitchell", 4.0), ("lanczos", 8.0)]

CASES = ([("base", f) for f in ALL] + [(s, f) for s in ("tile3-linear", "tile3-centre", "tile3-random", "narrow", "2x2", "1x1",
                                                         "crop", "clamp") for f in WIDE])
_oracle_cache, _product_cache = {}, {}


def spec_of(shape, filt):
    return SHAPES[shape](filter_type=filt[0], aa_pixelwidth=filt[1])


def oracle_render(O, shape, filt):
    """(rgba, weights, camera rays) of the oracle, rendered once per (shape, filter) and shared."""
    k = (shape, filt)
    if k not in _oracle_cache:
        rgba, w, ctr = O.OracleScene(spec_of(shape, filt), threads=4).render()
        rgba.setflags(write=False)
        w.setflags(write=False)
        _oracle_cache[k] = (rgba, w, int(ctr[0]))
    return _oracle_cache[k]


def product_render(Y, shape, filt, members=None):
    k = (shape, filt, members)
    if k not in _product_cache:
        _product_cache[k] = Y.render_spec(spec_of(shape, filt), members=members)
    return _product_cache[k]


def same_film(a, b):
    return np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1]))


def require_same_samples(Y, O, shape, members=None):
    """The preamble: the same spec under box 1.0 on both sides, bit-equal."""
    box = ("box", 1.0)
    assert same_film(product_render(Y, shape, box, members), oracle_render(O, shape, box)), "samples differ — not a film finding"


def describe(a, b):
    d = bits(a[0]) != bits(b[0])
    return "%d of %d colour values and %d of %d weights differ" % (d.sum(), d.size, (bits(a[1]) != bits(b[1])).sum(), b[1].size)


def test_exact_scene_is_three_constants_and_overshoots(oracle_built):
    """The premise: under box 1.0 every hit sample is one of three colours, and the signed lobes are exercised: a
    mitchell film overshoots the brightest sample."""
    rgba, w, rays = oracle_render(oracle_built, "part-linear", ("box", 1.0))     # 1 spp: the film is the samples
    cols = np.unique(rgba.reshape(-1, 4)[rgba.reshape(-1, 4)[:, 3] > 0], axis=0)
    assert rays == 23 * 17 and np.all(w == 1.0)
    want = {tuple(np.float32(c) * np.float32(e) for c in m.color) for m, e in
            zip(SHAPES["base"]().materials, FL.EMIT)}
    assert len(cols) == 3 and {tuple(c[:3]) for c in cols} == want
    brightest = max(max(c) for c in want)
    for f in (("mitchell", 1.0), ("mitchell", 1.5), ("mitchell", 4.0)):
        assert oracle_render(oracle_built, "base", f)[0][..., :3].max() > brightest, f


@pytest.mark.parametrize("shape", SPP1)
@pytest.mark.parametrize("filt", WIDE + [("mitchell", 1.5)], ids=fid)
def test_restatement_equals_the_oracle_film(oracle_built, shape, filt):
    """filmlib.splat, the numpy restatement of ImageFilm::addSample, over the oracle's own box 1.0 film of the
    scene (at one sample per pixel that film is the samples) against the oracle's film under the filter."""
    final, wt = restated(oracle_built, shape, filt)
    rgba, w, _ = oracle_render(oracle_built, shape, filt)
    assert np.array_equal(bits(wt), bits(w)) and np.array_equal(bits(final[-1]), bits(rgba))


def restated(O, shape, filt):
    s = spec_of(shape, filt).render
    samples = oracle_render(O, shape, ("box", 1.0))[0]
    return FL.splat(samples, FL.tile_list(s.width, s.height, s.tile_size, s.tiles_order), FL.film_setup(*filt))


# ---------------------------------------------------------------------------------------------------------------
# GPU: the films
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("shape,filt", CASES, ids=["%s-%s" % (s, fid(f)) for s, f in CASES])
def test_film_equals_the_oracle_bitwise(product, oracle_built, shape, filt):
    require_same_samples(product, oracle_built, shape)
    got, want = product_render(product, shape, filt), oracle_render(oracle_built, shape, filt)
    print(shape, fid(filt), "min weight", want[1].min(), "film range", want[0][..., :3].min(), want[0][..., :3].max())
    assert same_film(got, want), describe(got, want)
    if shape in SPP1:
        final, wt = restated(oracle_built, shape, filt)
        assert np.array_equal(bits(got[0]), bits(final[-1])) and np.array_equal(bits(got[1]), bits(wt))


ADAPTIVE_CASES = [("adaptive", ("mitchell", 1.5)), ("adaptive", ("lanczos", 8.0)), ("adaptive-curve", ("mitchell", 1.5))]


@pytest.mark.gpu
@pytest.mark.parametrize("shape,filt", ADAPTIVE_CASES, ids=["%s-%s" % (s, fid(f)) for s, f in ADAPTIVE_CASES])
def test_adaptive_passes_read_signed_films(product, oracle_built, shape, filt):
    """40x30, 1 + 2 + 2 samples over three passes: the threshold code (abscol2Bri, colorDifference) reads negative
    and overshooting colours, the resample flags feed the generic k_film's accumulate path.  The passes must
    resample some but not all of the film, and the same pixels on both sides."""
    require_same_samples(product, oracle_built, shape)
    got, want = product_render(product, shape, filt), oracle_render(oracle_built, shape, filt)
    print(shape, fid(filt), "camera rays: oracle", want[2], "product", got[2]["samples"])
    assert 1200 < want[2] < 6000
    assert got[2]["samples"] == want[2]
    assert same_film(got, want), describe(got, want)


@pytest.mark.gpu
@pytest.mark.parametrize("shape,filt", [("bands", ("lanczos", 8.0)), ("adaptive", ("mitchell", 1.5))],
                         ids=["bands-lanczos8", "adaptive-mitchell1.5"])
def test_device_group_halo_wider_than_a_band(product, oracle_built, shape, filt):
    """3 members: 23x10 gives bands of 3 or 4 rows under a forward reach of 4 (halo rows from beyond the neighbouring
    band); the adaptive case covers the row range of the flag exchange between passes."""
    require_same_samples(product, oracle_built, shape, members=3)
    one, three = product_render(product, shape, filt, members=1), product_render(product, shape, filt, members=3)
    want = oracle_render(oracle_built, shape, filt)
    assert same_film(one, want), describe(one, want)
    assert same_film(three, want), describe(three, want)


# ---------------------------------------------------------------------------------------------------------------
# GPU: the per-tile partial film with a backward-reaching filter
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("order", ["linear", "centre"])
@pytest.mark.parametrize("filt", PARTIAL_FILTERS, ids=fid)
def test_partial_film_with_backward_reach(product, oracle_built, order, filt):
    """putPixel shows a pixel as the one-thread render does when its tile finishes (ImageFilm::finishArea,
    imagefilm.cc:489-531): the film after the tiles up to its own have splatted.  With a backward reach a pixel
    also has sources in later tiles, so no order settles every pixel — not even the linear one."""
    shape = "part-" + order
    require_same_samples(product, oracle_built, shape)
    s = spec_of(shape, filt)
    W, H = s.render.width, s.render.height
    tiles = FL.tile_list(W, H, s.render.tile_size, order)
    after, wt = restated(oracle_built, shape, filt)
    assert FL.film_setup(*filt).reach_back > 0
    yi = product.Interface()
    scenes.apply(s, yi)
    per_tile, final, state, areas = {}, np.full((H, W, 4), np.nan, np.float32), {"cur": None}, []

    def highlight(aid, x0, y0, x1, y1):
        areas.append((aid, (x0, y0, x1, y1)))
        state["cur"] = aid

    def put(x, y, r, g, b, a):
        if state["cur"] is None:
            final[y, x] = (r, g, b, a)      # the final flush, after the last tile's flushArea
        else:
            per_tile[(x, y)] = (state["cur"], (r, g, b, a))

    def flush_area(aid, x0, y0, x1, y1):
        state["cur"] = None

    yi.render(put_pixel=put, flush_area=flush_area, highlight_area=highlight)
    film, wts = yi.film()
    yi.close()
    assert areas == list(enumerate(tiles))
    assert np.array_equal(bits(final), bits(film)) and np.array_equal(bits(film), bits(after[-1])) and np.array_equal(bits(wts), bits(wt))
    want = oracle_render(oracle_built, shape, filt)
    assert same_film((film, wts), want), describe((film, wts), want)
    assert len(per_tile) == W * H
    part, expect = np.empty((H, W, 4), np.float32), np.empty((H, W, 4), np.float32)
    for k, (x0, y0, x1, y1) in enumerate(tiles):
        expect[y0:y1, x0:x1] = after[k][y0:y1, x0:x1]
    for (x, y), (k, v) in per_tile.items():
        x0, y0, x1, y1 = tiles[k]
        assert x0 <= x < x1 and y0 <= y < y1
        part[y, x] = v
    assert np.array_equal(bits(part), bits(expect)), "%d pixels differ" % (bits(part) != bits(expect)).any(-1).sum()
    # unsettled pixels: a source in a later tile.  At one sample per pixel the samples sit at dx = dy = 0.5, whose
    # footprint reaches -roundToInt(0.5 - filterw) pixels back: 3 under lanczos 8.0 and mitchell 4.0 (filterw 4.0), none under
    # mitchell 1.5 (filterw 1.95: its reach_back of 1 needs dx < 0.45), which the linear order therefore still settles.
    back_at_centre = -FL._round_to_int(0.5 - float(np.float32(FL.film_setup(*filt).filterw)))
    assert back_at_centre == {("mitchell", 1.5): 0, ("mitchell", 4.0): 3, ("lanczos", 8.0): 3}[filt]
    unsettled = (bits(expect) != bits(after[-1])).any(-1)
    assert unsettled.any() == (order != "linear" or back_at_centre > 0) and not unsettled.all()
    assert (bits(part) != bits(film)).any(-1)[unsettled].all()
