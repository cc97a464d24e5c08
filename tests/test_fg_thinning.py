"""Final gathering's radiance-point thinning (integrator_photon_mapping.cc:560-572): the serial
greedy walk of the reference (a point still in use is kept and marks its related points unused)
and the round formulation the GPU runs (libyafaray_amd/csrc/fgthin.hip: keep / kill rounds over
the undecided points) give the same kept set — the lexicographically-first maximal independent
set of the relation "squared distance < maxrad and normals on the same side".  Checked here on
random point sets with numpy restatements of both; the second half of the file runs the kernels
themselves, their host twin and the oracle's walk against greedy() on inputs built for their edges
(tests/test_final_gather.py checks them through the images that depend on the kept set)."""
import numpy as np
import pytest


def related(pos, nrm, i, maxrad):
    v = pos - pos[i]
    d2 = (v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]
    nd = (nrm[:, 0] * nrm[i, 0] + nrm[:, 1] * nrm[i, 1]) + nrm[:, 2] * nrm[i, 2]
    return (d2 < maxrad) & (nd > 0)


def greedy(pos, nrm, maxrad):
    use = np.ones(len(pos), bool)
    kept = []
    for i in range(len(pos)):
        if use[i]:
            kept.append(i)
            use[related(pos, nrm, i, maxrad)] = False
    return kept


def rounds(pos, nrm, maxrad):
    n = len(pos)
    UND, KEPT, DEAD = 0, 1, 2
    state = np.zeros(n, np.int8)
    rel = [np.nonzero(related(pos, nrm, i, maxrad))[0] for i in range(n)]
    U = np.arange(n)
    r = 0
    while len(U):
        # keep: no undecided lower related point in the snapshot
        newk = [i for i in U if not np.any((rel[i] < i) & (state[rel[i]] == UND))]
        # kill: newly kept points mark their higher related points dead
        for i in newk:
            state[i] = KEPT
            hi = rel[i][rel[i] > i]
            state[hi] = DEAD
        U = np.array([i for i in U if state[i] == UND], dtype=np.int64)
        r += 1
        assert r <= n
    return list(np.nonzero(state == KEPT)[0]), r


@pytest.mark.parametrize("seed", range(6))
def test_rounds_equal_greedy(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(50, 400))
    pos = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    if seed % 2:
        pos[:, 2] = np.float32(0.25)          # points on a plane (as on the Cornell walls)
    nrm = rng.normal(size=(n, 3)).astype(np.float32)
    nrm /= np.linalg.norm(nrm, axis=1, keepdims=True)
    maxrad = np.float32(rng.uniform(0.01, 0.2))
    kept, r = rounds(pos, nrm, maxrad)
    assert kept == greedy(pos, nrm, maxrad)
    assert r >= 1


# ---------------------------------------------------------------------------------------------------------
# The kernels themselves (yafaray_amd_thinRadPoints: k_thin_keep / k_thin_kill, the clamped cell grid and the host
# round loop), the host twin (render.cc eliminateRadPoints, both grid paths) and the oracle's walk, each against
# greedy() above on inputs the final-gathering scenes do not reach: distances exactly on maxrad, perpendicular
# normals, duplicates, points on the bound, degenerate extents, crowded cells, counts that end inside a lane
# group / wave / block, long dependency chains, the "grid too large" refusal and scratch reuse.
# ---------------------------------------------------------------------------------------------------------
import functools  # noqa: E402

F = np.float32
UP = F(np.inf)


def unit_normals(rng, n):
    v = rng.normal(size=(n, 3))
    return (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(F)


def const_normals(n, v=(0, 0, 1)):
    return np.tile(np.asarray(v, F), (n, 1))


# ---- tie lattice: squared distances 0.0625, 0.125, 0.1875 between neighbours are exact in float32 ----
LATTICE_MAXRAD = [F(0.0625), np.nextafter(F(0.0625), UP), F(0.125), np.nextafter(F(0.125), UP), F(0.1875), np.nextafter(F(0.1875), UP)]
LATTICE_KEPT = [108, 35, 35, 18, 18, 15]      # a `<=` for the strict `<` would turn 108 into 35, 35 into 18, 18 into 15
LATTICE_ROUNDS = {0: 1, 1: 3}


def lattice_points():
    g = np.stack(np.meshgrid(np.arange(6), np.arange(6), np.arange(3), indexing="ij"), -1).reshape(-1, 3)
    pos = (g * 0.25).astype(F)
    np.random.default_rng(5).shuffle(pos)
    return pos, const_normals(len(pos))


# ---- normals: equal, opposite and exactly perpendicular (nd == 0 is unrelated), on coincident and near points ----
def normals_points():
    X, Y, Z = (1, 0, 0), (0, 1, 0), (0, 0, 1)
    neg = lambda v: tuple(-c for c in v)   # noqa: E731
    o, a, b = (0, 0, 0), (0.01, 0, 0), (0, 0.01, 0)
    rows = [(o, Z),        # 0 kept
            (o, Z),        # 1 duplicate of 0, equal normal: dead
            (o, neg(Z)),   # 2 duplicate, opposite normal: kept
            (o, X),        # 3 duplicate, perpendicular to 0 and 2: kept
            (a, X),        # 4 near 3, equal normal: dead
            (a, neg(X)),   # 5 near, opposite to 3, perpendicular to 0 and 2: kept
            (b, Y),        # 6 near, perpendicular to all kept so far: kept
            (b, Y),        # 7 duplicate of 6: dead
            (b, neg(Y)),   # 8 kept
            (a, Z),        # 9 near 0, equal normal: dead
            (b, neg(Z)),   # 10 near 2, equal normal: dead
            (o, neg(X))]   # 11 duplicate position, equal normal to 5 (near): dead
    return np.array([r[0] for r in rows], F), np.array([r[1] for r in rows], F)


NORMALS_KEPT = [0, 2, 3, 5, 6, 8]


# ---- chains: each point related to its two neighbours only, so every round decides one kept point ----
def chain_points(n, diagonal=False, reverse=False):
    i = np.arange(n, dtype=F)
    pos = np.stack([i * F(0.125)] * 3, 1) if diagonal else np.stack([i * F(0.25), 0 * i, 0 * i], 1)
    pos = pos.astype(F)
    return (pos[::-1].copy() if reverse else pos), const_normals(n)


CHAIN_MAXRAD = F(0.1)      # straight: neighbours 0.0625, next 0.25; diagonal: neighbours 3/64, next 3/16

# ---- shapes: counts that end inside a lane group (8), a wave (64), a block (256); degenerate extents ----
SHAPE_N = [1, 2, 7, 8, 9, 63, 64, 65, 255, 256, 257, 2049]
SHAPE_PLACE = ["cube", "plane", "line", "point"]


def shape_points(n, place):
    rng = np.random.default_rng(1000 * SHAPE_PLACE.index(place) + n)
    pos = rng.uniform(0, 1, (n, 3)).astype(F)
    if place == "cube":
        maxrad = 0.5 * n ** (-2.0 / 3.0)
    elif place == "plane":
        pos[:, 2] = F(0.25)
        maxrad = 0.5 / n
    elif place == "line":
        pos[:, 1:] = F(0.25)
        maxrad = 1.0 / (n * n)
    else:
        pos[:] = np.array([0.3, -0.2, 0.7], F)
        maxrad = 0.01
    return pos, unit_normals(rng, n), F(maxrad)


def dense_points():
    rng = np.random.default_rng(11)
    return rng.uniform(0, 0.05, (3000, 3)).astype(F), const_normals(3000), F(4e-4)


# ---- bound: points exactly on the minimum and maximum of every axis, the extent on a multiple of the cell (the
# float32 values around k * cell: where the division that sizes the grid and the multiplication that finds a
# cell round differently, only the clamp keeps the maximum inside the grid) ----
BOUND_MAXRAD = F(0.25)


def bound_extents():
    out = []
    for factor in (1.001, 1.0001):                   # the GPU's and the host twin's cell
        cell = np.sqrt(np.float64(BOUND_MAXRAD)) * factor + 1e-30
        for k in (1, 2, 3, 5, 8):
            e = F(k * cell)
            out += [np.nextafter(e, -UP), e, np.nextafter(e, UP)]
    return out


def bound_points(extent):
    corners = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], F)
    inward = np.where(corners > 0, F(-0.25), F(0.25))
    rows = [corners * extent]
    for off in ((1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 1)):
        rows.append(corners * extent + inward * np.asarray(off, F))
    pos = np.concatenate(rows).astype(F)
    np.random.default_rng(3).shuffle(pos)
    return pos, const_normals(len(pos))


# ---- refusal: a dense grid of ~10^9 cells (the GPU refuses, the twin takes its sparse path) and one between the
# twin's 2^24 and the GPU's 2^26 (the GPU serves, the twin takes its sparse path) ----
def cluster_points(spread, seed, n=60):
    rng = np.random.default_rng(seed)
    pos = rng.uniform(0, spread, (2 * n, 3)).astype(F)
    pos[n:, 0] += F(1000.0)
    return pos, const_normals(2 * n)


def refused_points():
    return cluster_points(3e-5, 21) + (F(1e-10),)


def mid_grid_points():
    return cluster_points(5e-3, 22) + (F(1e-6),)


def grid_cells(pos, maxrad, factor):
    cell = np.sqrt(np.float64(maxrad)) * factor + 1e-30
    ext = pos.max(0).astype(np.float64) - pos.min(0).astype(np.float64)
    return float(np.prod(np.floor(ext / cell) + 1.0))


def large_points():
    rng = np.random.default_rng(70)
    return rng.uniform(0, 1, (70000, 3)).astype(F), unit_normals(rng, 70000), F(4.5e-3)


def small_cases():
    c = {}
    lp = lattice_points()
    for k, m in enumerate(LATTICE_MAXRAD):
        c[f"lattice-{k}"] = lp + (m,)
    c["normals"] = normals_points() + (F(0.01),)
    c["chain-64"] = chain_points(64) + (CHAIN_MAXRAD,)
    c["chain-200"] = chain_points(200) + (CHAIN_MAXRAD,)
    c["chain-200-diagonal"] = chain_points(200, diagonal=True) + (CHAIN_MAXRAD,)
    c["chain-200-reversed"] = chain_points(200, reverse=True) + (CHAIN_MAXRAD,)
    for place in SHAPE_PLACE:
        for n in SHAPE_N:
            c[f"{place}-{n}"] = shape_points(n, place)
    c["dense"] = dense_points()
    for k, e in enumerate(bound_extents()):
        c[f"bound-{k}"] = bound_points(e) + (BOUND_MAXRAD,)
    c["refused"] = refused_points()
    c["mid-grid"] = mid_grid_points()
    return c


CASES = small_cases()


@functools.lru_cache(maxsize=None)
def want(name):
    """greedy() of a small case, computed once for the CPU and the GPU tests."""
    pos, nrm, maxrad = CASES[name]
    return greedy(pos, nrm, maxrad)


@functools.lru_cache(maxsize=None)
def want_rounds(name):
    pos, nrm, maxrad = CASES[name]
    kept, r = rounds(pos, nrm, maxrad)
    assert kept == want(name)
    return r


@functools.lru_cache(maxsize=None)
def want_large():
    from oracle import oracle as O
    pos, nrm, maxrad = large_points()
    return O.thin_rad_points(pos, nrm, maxrad).tolist()


def test_cases_are_what_they_claim():
    """The counts worked out with numpy when the cases were chosen; a case that degenerates cannot pass silently."""
    for k, (nk, m) in enumerate(zip(LATTICE_KEPT, LATTICE_MAXRAD)):
        assert len(want(f"lattice-{k}")) == nk, (k, float(m))
    for k, r in LATTICE_ROUNDS.items():
        assert want_rounds(f"lattice-{k}") == r
    assert want("normals") == NORMALS_KEPT
    for name, n in (("chain-64", 64), ("chain-200", 200), ("chain-200-diagonal", 200), ("chain-200-reversed", 200)):
        assert want(name) == list(range(0, n, 2)) and want_rounds(name) == n // 2, name
    for n in SHAPE_N:
        k = want(f"point-{n}")
        assert k[0] == 0 and (n < 7 or 1 < len(k) < n), (n, len(k))      # coincident points: the normals alone decide
    for place in ("cube", "plane", "line"):
        k = want(f"{place}-2049")
        assert 0.2 * 2049 < len(k) < 0.9 * 2049, (place, len(k))
    assert 1 < len(want("dense")) < 3000
    pos, _, maxrad = CASES["refused"]
    assert grid_cells(pos, maxrad, 1.001) > 2 ** 26 and grid_cells(pos, maxrad, 1.0001) > 2 ** 24
    assert 1 < len(want("refused")) < len(pos)
    pos, _, maxrad = CASES["mid-grid"]
    assert grid_cells(pos, maxrad, 1.001) <= 2 ** 26 and grid_cells(pos, maxrad, 1.0001) > 2 ** 24
    assert 1 < len(want("mid-grid")) < len(pos)
    for name in CASES:
        if name.startswith("bound-"):
            assert 1 < len(want(name)) < len(CASES[name][0]), name


@pytest.mark.parametrize("name", sorted(CASES))
def test_oracle_and_host_twin_equal_greedy(product, oracle_built, name):
    """The oracle's walk (yc_thin_rad_points, the body its render runs) and the host twin (mode "host": render.cc
    eliminateRadPoints, dense grid or hashed cells) against greedy(); no GPU involved."""
    pos, nrm, maxrad = CASES[name]
    assert oracle_built.thin_rad_points(pos, nrm, maxrad).tolist() == want(name)
    yi = product.Interface()
    kept, r = yi.thin_rad_points(pos, nrm, maxrad, "host")
    yi.close()
    assert kept.tolist() == want(name) and r == -1


def test_large_case_oracle_equals_host_twin(product, oracle_built):
    pos, nrm, maxrad = large_points()
    yi = product.Interface()
    kept, r = yi.thin_rad_points(pos, nrm, maxrad, "host")
    yi.close()
    assert kept.tolist() == want_large() and r == -1
    assert 0.03 * len(pos) < len(kept) < 0.08 * len(pos), len(kept)
    # the oracle export against greedy() on the first 3,000 of these points (greedy() itself is too slow for all)
    assert oracle_built.thin_rad_points(pos[:3000], nrm[:3000], F(0.02)).tolist() == greedy(pos[:3000], nrm[:3000], F(0.02))


@pytest.fixture(scope="module")
def gpu_iface(product):
    yi = product.Interface()      # one interface for the module: every call reuses the renderer's thinning scratch
    yield yi
    yi.close()


def check_gpu(yi, pos, nrm, maxrad, expect, expect_rounds=None):
    kept, r = yi.thin_rad_points(pos, nrm, maxrad, "render")
    assert r >= 1, "the GPU did not serve this point set"
    assert kept.tolist() == expect
    kept_g, r_g = yi.thin_rad_points(pos, nrm, maxrad, "gpu")
    assert kept_g.tolist() == expect and r_g == r
    kept_h, r_h = yi.thin_rad_points(pos, nrm, maxrad, "host")
    assert kept_h.tolist() == expect and r_h == -1
    if expect_rounds is not None:
        assert r == expect_rounds


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(n for n in CASES if n != "refused"))
def test_gpu_thinning_equals_greedy(gpu_iface, name):
    pos, nrm, maxrad = CASES[name]
    check_gpu(gpu_iface, pos, nrm, maxrad, want(name), want_rounds(name) if len(pos) <= 2000 else None)


@pytest.mark.gpu
def test_gpu_lattice_counts(gpu_iface):
    """The strict `<` on exact ties: the kept counts at and one ulp above each lattice distance."""
    pos, nrm = lattice_points()
    got = [len(gpu_iface.thin_rad_points(pos, nrm, m, "gpu")[0]) for m in LATTICE_MAXRAD]
    assert got == LATTICE_KEPT
    assert [gpu_iface.thin_rad_points(pos, nrm, LATTICE_MAXRAD[k], "gpu")[1] for k in (0, 1)] == [1, 3]


@pytest.mark.gpu
def test_gpu_refuses_a_grid_too_large(gpu_iface):
    pos, nrm, maxrad = CASES["refused"]
    with pytest.raises(RuntimeError, match="too large for the GPU"):
        gpu_iface.thin_rad_points(pos, nrm, maxrad, "gpu")
    for mode in ("render", "host"):
        kept, r = gpu_iface.thin_rad_points(pos, nrm, maxrad, mode)
        assert kept.tolist() == want("refused") and r == -1, mode
    # the refusal leaves the renderer usable
    check_gpu(gpu_iface, *CASES["lattice-1"], want("lattice-1"), 3)


@pytest.mark.gpu
def test_gpu_scratch_reuse_between_sizes(product):
    yi = product.Interface()
    try:
        big_a = shape_points(2049, "cube")
        small = shape_points(7, "cube")
        rng = np.random.default_rng(99)
        big_b = (rng.uniform(-2, 2, (2049, 3)).astype(F), unit_normals(rng, 2049), F(0.05))
        for pos, nrm, maxrad in (big_a, small, big_b):
            kept, r = yi.thin_rad_points(pos, nrm, maxrad, "gpu")
            assert kept.tolist() == greedy(pos, nrm, maxrad) and r >= 1
    finally:
        yi.close()


@pytest.mark.gpu
def test_gpu_large_case_equals_oracle(gpu_iface):
    """70,000 points (274 blocks of k_thin_cells, 2,188 of k_thin_keep; the compaction over several tiles)."""
    pos, nrm, maxrad = large_points()
    kept, r = gpu_iface.thin_rad_points(pos, nrm, maxrad, "gpu")
    assert kept.tolist() == want_large() and r >= 1


@pytest.mark.gpu
def test_gpu_empty_and_bad_arguments(gpu_iface):
    kept, r = gpu_iface.thin_rad_points(np.zeros((0, 3), F), np.zeros((0, 3), F), F(0.1), "gpu")
    assert len(kept) == 0 and r == 0
    L, h = gpu_iface.L, gpu_iface.h
    assert not L.yafaray_amd_thinRadPoints(h, None, None, 3, 0.1, 0, None, None, None)
    assert not L.yafaray_amd_thinRadPoints(h, None, None, 0, 0.1, 7, None, None, None)
