"""Photon-map queries on their own: the k-NN gather (PhotonMap::gather: pkdtree.h:225-292 + photon.cc:31-52) and the
nearest lookup (PhotonMap::findNearest, photon.cc:136-142) of every GPU form, on maps and query points built for
their edges, against two CPU references.

  * Brute force (numpy, below): for every query the squared distance to every photon in float32 with the kernels'
    expression, v = photon - p; (vx vx + vy vy) + vz vz.  It fixes what any correct lookup returns: found =
    min(k, #{d2 < r2}), the final radius (the k-th smallest d2, or r2 unchanged), the multiset of distances, and the
    photons themselves except among those tied at the k-th distance.
  * The sequential lookup (oracle yc_photon_gather / yc_photon_nearest, the functions the oracle's renders run): the
    reference's visit order and heap moves, so the heap in array order and the identity of tied photons.

The unmarked tests prove the oracle's exports against brute force on every family and the families' own stated
properties.  The GPU tests run yafaray_amd_queryPhotons (Interface.query_photons): every kind must equal the
sequential lookup bit for bit, heap order and tied identities included, and satisfy the brute-force conditions.

Tolerances: none.  Every comparison is of bits; the lookups only compare, copy and square-and-add floats, and both
references form d2 with the same three products and two sums, uncontracted."""
import functools

import numpy as np
import pytest

F = np.float32


# ---------------------------------------------------------------------------------------------
# brute force
# ---------------------------------------------------------------------------------------------
def d2_rows(pos, qs):
    """(m, n) float32 squared distances, the kernels' expression (no contraction: separate ufuncs)"""
    with np.errstate(over="ignore", under="ignore"):   # (the extreme families overflow to +inf and underflow on purpose)
        v = pos[None, :, :] - qs[:, None, :]
        return (v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1]) + v[..., 2] * v[..., 2]


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


class Expect:
    """what brute force fixes for one (map, queries, k, r2): per query the count, the final radius, the `found`
    smallest distances in ascending order, the photons strictly below the k-th distance, the photons at it, and
    whether the choice among those is free"""

    def __init__(self, pos, qs, k, r2):
        r2 = F(r2)
        self.pos, self.qs, self.k, self.r2 = pos, qs, k, r2
        self.found, self.radius, self.small, self.strict, self.at_kth, self.amb, self.inside = [], [], [], [], [], [], []
        for q in range(len(qs)):
            d = d2_rows(pos, qs[q:q + 1])[0]
            ins = np.nonzero(d < r2)[0]
            self.inside.append(len(ins))
            f = min(k, len(ins))
            di = d[ins]
            if len(ins) > k:
                kth = np.partition(di, k - 1)[k - 1]
                strict = ins[di < kth]
                at = ins[di == kth]
                small = np.sort(np.concatenate([di[di < kth], np.full(f - len(strict), kth, F)]))
            else:
                kth = di.max() if f == k else r2
                strict = ins[di < kth] if f == k else ins
                at = ins[di == kth] if f == k else ins[:0]
                small = np.sort(di)
            self.found.append(f)
            self.radius.append(F(kth) if f == k else r2)
            self.small.append(small.astype(F))
            self.strict.append(set(strict.tolist()))
            self.at_kth.append(set(at.tolist()))
            self.amb.append(f == k and len(strict) + len(at) > f)
        self.found = np.array(self.found, np.int32)
        self.radius = np.array(self.radius, F)
        self.amb = np.array(self.amb, bool)

    def check(self, res, what):
        """the brute-force conditions on a lookup's (found, radius2, idx, dist)"""
        found, rad, idx, dist = res
        n = len(self.pos)
        assert np.array_equal(found, self.found), f"{what}: found differs from min(k, #inside) at {np.nonzero(found != self.found)[0][:8]}"
        assert np.array_equal(bits(rad), bits(self.radius)), f"{what}: final radius at {np.nonzero(bits(rad) != bits(self.radius))[0][:8]}"
        for q in range(len(self.qs)):
            f = int(found[q])
            gi, gd = idx[q, :f].astype(np.int64), dist[q, :f]
            assert (gi < n).all() and len(set(gi.tolist())) == f, f"{what}: query {q}: indices not distinct photons"
            own = d2_rows(self.pos[gi], self.qs[q:q + 1])[0] if f else np.zeros(0, F)
            assert np.array_equal(bits(own), bits(gd)), f"{what}: query {q}: a reported distance is not its photon's"
            assert np.array_equal(bits(np.sort(gd)), bits(self.small[q])), f"{what}: query {q}: not the {f} smallest distances"
            got = set(gi.tolist())
            # identity is free only among the photons at the k-th distance, and only when more qualify than fit
            assert self.strict[q] <= got and got <= (self.strict[q] | self.at_kth[q]), f"{what}: query {q}: wrong photon set"
            if not self.amb[q]:
                assert got == (self.strict[q] | self.at_kth[q]), f"{what}: query {q}: wrong photon set without a tie"
            assert (idx[q, f:] == 0xffffffff).all() and (bits(dist[q, f:]) == 0).all(), f"{what}: query {q}: slots beyond found"


def nearest_expect(pos, dirs, qs, ns, r2):
    """per query (smallest facing d2 below r2 or None, the photons at it)"""
    out = []
    for q in range(len(qs)):
        d = d2_rows(pos, qs[q:q + 1])[0]
        facing = ((dirs[:, 0] * ns[q, 0] + dirs[:, 1] * ns[q, 1]) + dirs[:, 2] * ns[q, 2]) > 0
        ok = facing & (d < F(r2))
        if not ok.any():
            out.append((None, set()))
            continue
        best = d[ok].min()
        out.append((best, set(np.nonzero(ok & (d == best))[0].tolist())))
    return out


def check_nearest(exp, got, what):
    for q, (best, who) in enumerate(exp):
        if best is None:
            assert got[q] == -1, f"{what}: query {q}: {got[q]} where no photon qualifies"
        else:
            assert int(got[q]) in who, f"{what}: query {q}: {got[q]} is not a nearest facing photon {sorted(who)[:4]}"


# ---------------------------------------------------------------------------------------------
# families
# ---------------------------------------------------------------------------------------------
SHAPES = ("cube", "plane", "line", "lattice", "dup4", "octaves")


@functools.lru_cache(maxsize=None)
def make_map(shape, n, seed=0):
    """n photon positions: what each shape is for is written in profiles/photon_query_parity.md"""
    rng = np.random.default_rng(1000 * SHAPES.index(shape) + n + 7919 * seed)
    if shape == "cube":
        p = rng.uniform(0, 1, (n, 3))
    elif shape == "plane":            # one constant coordinate: two axes carry every split, ties on the third
        p = rng.uniform(0, 1, (n, 3))
        p[:, 2] = 0.25
    elif shape == "line":             # one axis carries every split
        p = np.zeros((n, 3))
        p[:, 0] = rng.uniform(0, 1, n)
        p[:, 1], p[:, 2] = 0.5, -0.25
    elif shape == "lattice":          # integer coordinates: exact distance ties, coordinates equal to split values
        side = max(1, int(np.ceil(n ** (1 / 3))))
        g = np.stack(np.meshgrid(np.arange(side), np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 3)
        p = g[rng.permutation(len(g))[:n]].astype(np.float64)
    elif shape == "dup4":             # every point four times: zero distances between photons, ties by index
        u = rng.uniform(0, 1, ((n + 3) // 4, 3))
        p = np.repeat(u, 4, axis=0)[rng.permutation(4 * len(u))][:n]
    elif shape == "octaves":          # distances from the origin spread over 2^-20 .. 2^20
        u = rng.normal(size=(n, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        p = u * np.exp2(rng.uniform(-20, 20, (n, 1)))
    else:
        raise KeyError(shape)
    p = np.ascontiguousarray(p, F)
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def make_queries(shape, n, m=96, seed=0):
    """m query points for a map: random inside and well outside the bound, exactly at photons, coordinates on split
    planes of the built tree, lattice midpoints — in this order, cyclically"""
    from oracle import oracle as O
    pos = make_map(shape, n, seed)
    rng = np.random.default_rng(77 + 1000 * SHAPES.index(shape) + n + m)
    lo, hi = pos.min(0).astype(np.float64), pos.max(0).astype(np.float64)
    ext = np.maximum(hi - lo, 1e-3)
    nodes, _ = O.photon_tree(pos)
    interior = np.nonzero((nodes[:, 1] & 3) != 3)[0]
    qs = np.zeros((m, 3), F)
    for i in range(m):
        kind = i % 6
        if shape == "octaves" and kind == 0:   # the centre of the spread and points next to it: 40 octaves of distances each
            q = np.zeros(3) if i % 12 == 0 else rng.normal(size=3) * np.exp2(-24)
        elif shape == "octaves" and kind == 5:
            q = rng.normal(size=3) * np.exp2(rng.uniform(-20, 20))
        elif kind == 0:
            q = rng.uniform(lo, hi)
        elif kind == 1:
            q = (lo + hi) / 2 + rng.choice([-1, 1], 3) * ext * rng.uniform(3, 10, 3)
        elif kind == 2:
            q = pos[rng.integers(n)].astype(np.float64)
        elif kind == 3 and len(interior):      # one coordinate exactly on a split plane (pa <= split_val)
            nd = interior[rng.integers(len(interior))]
            q = rng.uniform(lo, hi)
            q[nodes[nd, 1] & 3] = nodes[nd:nd + 1, 0].view(F)[0]
        elif kind == 4 and len(interior):      # every coordinate on some split plane of its axis (or a photon's coordinate)
            q = pos[rng.integers(n)].astype(np.float64)
            for nd in interior[rng.integers(len(interior), size=6)]:
                q[nodes[nd, 1] & 3] = nodes[nd:nd + 1, 0].view(F)[0]
        else:                                  # midpoints of the unit lattice: 2, 4 or 8 nearest lattice points tie
            q = np.floor(rng.uniform(lo, hi + 1)) + rng.choice([0.0, 0.5], 3)
        if shape == "lattice" and kind != 1:   # on the lattice and its half steps: shells of equidistant photons
            q = np.round(np.asarray(q, np.float64) * 2) / 2
        qs[i] = q
    qs.setflags(write=False)
    return qs


def kcount_family(k, clusters=12):
    """clusters of k - 1, k and k + 1 photons (in turn) within 0.4 of their centres, centres 100 apart, one query at
    each centre; with r2 = 1 exactly those photons are inside"""
    rng = np.random.default_rng(4242 + k)
    pos, qs, want = [], [], []
    for c in range(clusters):
        centre = np.array([100.0 * c, -50.0 * (c % 3), 25.0 * (c % 2)])
        cnt = max(0, k - 1 + c % 3)
        u = rng.normal(size=(cnt, 3))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        pos.append(centre + u * rng.uniform(0.01, 0.4, (cnt, 1)))
        qs.append(centre)
        want.append(cnt)
    pos = np.ascontiguousarray(np.concatenate(pos), F)
    order = rng.permutation(len(pos))
    return pos[order], np.ascontiguousarray(qs, F), np.array(want), F(1.0)


def extreme_family(which):
    """maps whose distances leave the comfortable range (the walk's 16-bit keys round distances up, towards +inf at
    the top of the float range; its radius is a bit pattern): `huge` has squared distances up to the largest finite
    floats and beyond (+inf: never inside any radius), `tiny` has subnormal and zero ones.  Returns (pos, queries,
    radii)."""
    rng = np.random.default_rng(99 + len(which))
    scale = {"huge": 9e18, "tiny": 3e-22}[which]
    pos = (rng.uniform(-1, 1, (3000, 3)) * scale).astype(F)
    qs = np.concatenate([rng.uniform(-1, 1, (40, 3)) * scale, pos[rng.integers(len(pos), size=24)]]).astype(F)
    radii = {"huge": [F(1e37), F(3.0e38), F(np.finfo(F).max), F(np.inf)], "tiny": [F(1e-45), F(3e-43), F(1e-38), F(1e30)]}[which]
    return pos, qs, radii


def shell_family(n):
    """n photons in a thin shell about the origin, queries at and next to the origin: every squared distance lies in
    (1, 1 + 2^-7), so each rounds up to the same 16-bit key, 1 + 2^-7.  The register walk's bound is the k-th
    smallest key, so it never drops below 1 + 2^-7: the walk accepts and logs every photon (no subtree is pruned
    either: a plane is never farther than the photons behind it)."""
    rng = np.random.default_rng(31 + n)
    u = rng.normal(size=(n, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    pos = (u * rng.uniform(1.0005, 1.003, (n, 1))).astype(F)
    qs = np.concatenate([np.zeros((1, 3)), rng.normal(size=(3, 3)) * 1e-5]).astype(F)
    d = d2_rows(pos, qs)
    assert d.min() > 1 and d.max() < 1 + 2.0 ** -7
    return pos, qs


DEEP_N, DEEP_M = 600_000, 256


@functools.lru_cache(maxsize=None)
def deep_map():
    rng = np.random.default_rng(600)
    pos = rng.uniform(0, 1, (DEEP_N, 3)).astype(F)
    qs = np.concatenate([rng.uniform(0, 1, (DEEP_M - 32, 3)), pos[rng.integers(DEEP_N, size=32)]]).astype(F)
    return pos, qs


# The walk stacks one far child per interior node of the path it descends, so a path of 20 interior nodes (the deep
# map: deepest level 20) fills stack levels 0 - 19, all in LDS, although pm_stack = 21 attaches a spill column.  The
# spill map has leaves on level 21: a first descent through 21 interior nodes with an unbounded radius (every far
# child is stacked while fewer than k photons are accepted) writes level 20 to the HBM column and pops it back.
SPILL_N, SPILL_M = 1_300_000, 64


@functools.lru_cache(maxsize=None)
def spill_map():
    rng = np.random.default_rng(1300)
    pos = rng.uniform(0, 1, (SPILL_N, 3)).astype(F)
    qs = np.concatenate([rng.uniform(0, 1, (SPILL_M - 16, 3)), pos[rng.integers(SPILL_N, size=16)]]).astype(F)
    return pos, qs


def first_descent_interiors(nodes, q):
    """interior nodes on the path the lookups descend first for point q (pa <= split goes left)"""
    cur, count = 0, 0
    while (nodes[cur, 1] & 3) != 3:
        axis = int(nodes[cur, 1] & 3)
        cur = cur + 1 if q[axis] <= nodes[cur:cur + 1, 0].view(F)[0] else int(nodes[cur, 1] >> 2)
        count += 1
    return count


def radii_for(pos, qs, k):
    """squared radii: below every distance, bit-equal to one photon's d2, a mid value, unbounded"""
    d = d2_rows(pos, qs[:32])
    kk = min(k, len(pos)) - 1
    kth = np.sort(d, axis=1)[:, kk]
    pick = d[0][np.argsort(d[0], kind="stable")[min(2, len(pos) - 1)]]     # query 0's third nearest photon, exactly
    return [F(d.min() / 2), F(pick), F(np.median(kth)), F(1e30)]


@functools.lru_cache(maxsize=None)
def expect_for(shape, n, m, k, r2b):
    return Expect(make_map(shape, n), make_queries(shape, n, m), k, np.uint32(r2b).view(F))


@functools.lru_cache(maxsize=None)
def oracle_for(shape, n, m, k, r2b):
    from oracle import oracle as O
    return O.photon_gather(make_map(shape, n), make_queries(shape, n, m), k, np.uint32(r2b).view(F))


def rbits(r):
    return int(np.array([r], F).view(np.uint32)[0])


def sizes_for(k):
    return sorted({1, 2, 3, max(1, k - 1), k, k + 1, 257})


def unit_dirs(n, seed):
    rng = np.random.default_rng(seed)
    u = rng.normal(size=(n, 3))
    return np.ascontiguousarray(u / np.linalg.norm(u, axis=1, keepdims=True), F)


# ---------------------------------------------------------------------------------------------
# CPU: the oracle's exports against brute force, and the families' stated properties
# ---------------------------------------------------------------------------------------------
def assert_same(a, b, what):
    for x, y, name in zip(a, b, ("found", "radius2", "idx", "dist")):
        x, y = np.asarray(x), np.asarray(y)
        same = np.array_equal(x.view(np.uint32) if x.dtype == F else x, y.view(np.uint32) if y.dtype == F else y)
        if not same:
            bad = np.nonzero((x.view(np.uint32) if x.dtype == F else x) != (y.view(np.uint32) if y.dtype == F else y))
            raise AssertionError(f"{what}: {name} differs from the sequential lookup at {[b[:6].tolist() for b in bad]}")


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_gather_equals_brute_force(oracle_built, shape):
    k = 7
    for n in sizes_for(k) + [5000]:
        pos, qs = make_map(shape, n), make_queries(shape, n)
        for r2 in radii_for(pos, qs, k):
            expect_for(shape, n, 96, k, rbits(r2)).check(oracle_for(shape, n, 96, k, rbits(r2)), f"oracle {shape} n={n} r2={r2}")


@pytest.mark.parametrize("k", [1, 2, 50, 64, 65, 100])
def test_oracle_gather_k_sweep(oracle_built, k):
    for shape, n in (("cube", 5000), ("lattice", 257), ("dup4", 257)):
        pos, qs = make_map(shape, n), make_queries(shape, n)
        for r2 in radii_for(pos, qs, k):
            expect_for(shape, n, 96, k, rbits(r2)).check(oracle_for(shape, n, 96, k, rbits(r2)), f"oracle {shape} n={n} k={k} r2={r2}")


@pytest.mark.parametrize("shape", SHAPES)
def test_oracle_nearest_equals_brute_force(oracle_built, shape):
    for n in (1, 2, 3, 257, 5000):
        pos, qs = make_map(shape, n), make_queries(shape, n)
        dirs, ns = unit_dirs(n, 5), unit_dirs(len(qs), 6)
        for r2 in radii_for(pos, qs, 1):
            got = oracle_built.photon_nearest(pos, dirs, qs, ns, r2)
            check_nearest(nearest_expect(pos, dirs, qs, ns, r2), got, f"oracle nearest {shape} n={n} r2={r2}")


def test_generic_family_has_no_ties():
    """nothing is excused on the generic family: no query has more photons at its k-th distance than fit"""
    for n in (257, 5000):
        for k in (1, 7, 50, 64):
            pos, qs = make_map("cube", n), make_queries("cube", n)
            for r2 in radii_for(pos, qs, k):
                assert not expect_for("cube", n, 96, k, rbits(r2)).amb.any()


def test_lattice_family_ties_on_most_queries():
    for n, k in ((257, 7), (5000, 7), (257, 2)):
        e = expect_for("lattice", n, 96, k, rbits(F(1e30)))
        assert e.amb.mean() > 0.5, (n, k, e.amb.mean())


@pytest.mark.parametrize("k", [2, 7, 50, 64])
def test_kcount_family_counts(oracle_built, k):
    pos, qs, want, r2 = kcount_family(k)
    e = Expect(pos, qs, k, r2)
    assert e.inside == want.tolist() and set(want.tolist()) == {k - 1, k, k + 1}
    assert not e.amb.any()
    e.check(oracle_built.photon_gather(pos, qs, k, r2), f"oracle kcount k={k}")


@pytest.mark.parametrize("which", ["huge", "tiny"])
def test_oracle_extreme_distances(oracle_built, which):
    pos, qs, radii = extreme_family(which)
    d = d2_rows(pos, qs)
    if which == "huge":
        assert np.isinf(d).any() and (d[np.isfinite(d)] > 1e38).any()
    else:
        assert ((d > 0) & (d < np.finfo(F).tiny)).any() and (d == 0).any()
    for k in (1, 7, 64):
        for r2 in radii:
            Expect(pos, qs, k, r2).check(oracle_built.photon_gather(pos, qs, k, r2), f"oracle {which} k={k} r2={r2}")


def test_deep_map_depth(oracle_built):
    """600 000 photons: 21 tree levels (deepest level 20), one more than the walk keeps in LDS"""
    pos, qs = deep_map()
    _, depth = oracle_built.photon_tree(pos)
    assert depth + 1 > 20
    e = Expect(pos, qs[:24], 50, F(1e30))
    assert not e.amb.any()
    e.check(oracle_built.photon_gather(pos, qs[:24], 50, F(1e30)), "oracle deep")


def test_spill_map_descends_21_levels(oracle_built):
    """1 300 000 photons: leaves on level 21, and a good share of the queries descend through 21 interior nodes first,
    one more than the walk's LDS stack levels"""
    pos, qs = spill_map()
    nodes, depth = oracle_built.photon_tree(pos)
    assert depth == 21
    deep = sum(first_descent_interiors(nodes, q) == 21 for q in qs)
    assert deep >= SPILL_M // 8, deep
    spill_expect().check(spill_oracle(), "oracle spill map")


@functools.lru_cache(maxsize=None)
def spill_oracle():
    from oracle import oracle as O
    pos, qs = spill_map()
    return O.photon_gather(pos, qs, 50, F(1e30))


@functools.lru_cache(maxsize=None)
def spill_expect():
    pos, qs = spill_map()
    return Expect(pos, qs, 50, F(1e30))


# ---------------------------------------------------------------------------------------------
# GPU
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def yi(product):
    it = product.Interface()
    yield it
    it.close()


def gpu_gather(yi, pos, qs, kind, k, r2, **kw):
    r = yi.query_photons(pos, qs, kind, k=k, radius2=r2, **kw)
    return (r["found"], r["radius2"], r["idx"], r["dist"]), r


def check_family(yi, shape, n, m, kind, k, r2, **kw):
    pos, qs = make_map(shape, n), make_queries(shape, n, m)
    what = f"kind {kind} {shape} n={n} m={m} k={k} r2={r2!r} {kw}"
    got, r = gpu_gather(yi, pos, qs, kind, k, r2, **kw)
    assert_same(got, oracle_for(shape, n, m, k, rbits(r2)), what)
    expect_for(shape, n, m, k, rbits(r2)).check(got, what)
    return r


def experiments_built():
    import libyafaray_amd as Y
    return "YAF_EXPERIMENTS" in Y.build_info()


GATHER_KINDS = (0, 1, 2, 3, 4)


def refused_without_experiments(yi, kind):
    """kind 5 (the bounded walk) exists in experiments builds; elsewhere the seam must refuse it, and the case ends"""
    if kind != 5 or experiments_built():
        return False
    with pytest.raises(RuntimeError, match="experiments builds only"):
        yi.query_photons(make_map("cube", 3), make_queries("cube", 3, 1), 5, k=1)
    return True


@pytest.mark.gpu
@pytest.mark.parametrize("kind", GATHER_KINDS)
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_small_maps(yi, shape, kind):
    """every shape at n = 1, 2, 3, k - 1, k, k + 1 and 257 photons, the four radii"""
    k = 7
    for n in sizes_for(k):
        for r2 in radii_for(make_map(shape, n), make_queries(shape, n), k):
            check_family(yi, shape, n, 96, kind, k, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,k", [(kind, k) for kind in (3, 4) for k in (1, 2, 7, 50, 63, 64)] +
                         [(kind, k) for kind in (1, 2) for k in (1, 2, 7, 50, 63, 64, 65, 100)])
def test_gather_k_sweep(yi, kind, k):
    for shape, n in (("cube", 5000), ("lattice", 257), ("dup4", 257), ("octaves", 5000)):
        for r2 in radii_for(make_map(shape, n), make_queries(shape, n), k):
            r = check_family(yi, shape, n, 96, kind, k, r2)
            assert r["counters"]["path"] == kind


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (1, 2, 3, 4))
@pytest.mark.parametrize("shape", SHAPES)
def test_gather_5000(yi, shape, kind):
    for k in (7, 50):
        check_family(yi, shape, 5000, 96, kind, k, F(1e30))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("k", [2, 7, 50, 64])
def test_gather_kcount_family(yi, kind, k):
    """exactly k - 1, k and k + 1 photons inside the radius"""
    if refused_without_experiments(yi, kind):
        return
    pos, qs, _, r2 = kcount_family(k)
    from oracle import oracle as O
    got, _ = gpu_gather(yi, pos, qs, kind, k, r2)
    assert_same(got, O.photon_gather(pos, qs, k, r2), f"kind {kind} kcount k={k}")
    Expect(pos, qs, k, r2).check(got, f"kind {kind} kcount k={k}")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (0, 1, 2, 3, 4, 5))
def test_gather_query_counts_and_segments(yi, kind):
    """m = 1, 63, 64, 65 and enough for a second trip of every request loop (the walk serves 1024 requests of a
    segment per trip, the gather 256; the pre-gather's grid of n_seg x 256 lanes strides over all 1100 points when
    n_seg is 1 or 3, with its stack column at that stride), over 1, 3 and the largest number of segments"""
    if refused_without_experiments(yi, kind):
        return
    max_seg = yi.query_photons(make_map("cube", 3), make_queries("cube", 3, 1), 1)["counters"]["max_seg"]
    assert max_seg >= 3
    for m in (1, 63, 64, 65):
        for n_seg in (1, 3, max_seg):
            check_family(yi, "cube", 257, m, kind, 7, F(1e30), n_seg=n_seg)
    for n_seg in (1, 3, max_seg):
        r = check_family(yi, "lattice", 257, 1100, kind, 7, F(1e30), n_seg=n_seg)
        assert r["counters"]["photons"] == 7 * 1100


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (3, 4, 5))
@pytest.mark.parametrize("k", [2, 50, 64])
def test_log_overflow_falls_back(yi, kind, k):
    """log_cap = k: every request that accepts more than k photons overflows its log and is looked up again — with the
    LDS heap (packed) or the heap in the request's own log (split); the answers do not change"""
    if refused_without_experiments(yi, kind):
        return
    for shape, n in (("cube", 5000), ("lattice", 257)):
        r = check_family(yi, shape, n, 96, kind, k, F(1e30), log_cap=k, want_log=True)
        c = r["counters"]
        assert c["log_cap"] == k and c["overflows"] > 0
        assert c["overflows"] == int((r["log_n"] > k).sum())
        d = check_family(yi, shape, n, 96, kind, k, F(1e30), want_log=True)
        assert d["counters"]["log_cap"] == 512 and d["counters"]["overflows"] == int((d["log_n"] > 512).sum())
        # the raw log: every photon the lookup keeps was logged with its distance, in pairs with an odd tail
        for q in range(96):
            na = int(d["log_n"][q])
            if na > 512:
                continue
            logged = {(int(a), int(b)) for a, b in d["log_e"][q, :na]}
            f = int(d["found"][q])
            kept = set(zip(d["idx"][q, :f].tolist(), bits(d["dist"][q, :f]).tolist()))
            assert kept <= logged and len(logged) == na, (shape, q)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (0, 1, 2, 3, 4))
def test_deep_map_spills(yi, kind):
    """pm_stack = 21: the walk keeps 20 levels in LDS and gets a spill column for the last; an unbounded radius pushes
    every level's far child before k photons are found (20 of them: test_spill_levels_are_used fills the 21st)"""
    pos, qs = deep_map()
    k = 50
    got, r = gpu_gather(yi, pos, qs, kind, k, F(1e30))
    c = r["counters"]
    assert c["pm_stack"] >= 21 and c["depth"] == c["pm_stack"] - 1
    if kind not in (1, 2):
        assert c["spill"] == 1 and c["pm_stack"] > c["lds_levels"] == 20, c
    assert_same(got, deep_oracle(), f"kind {kind} deep map")
    deep_expect().check(got, f"kind {kind} deep map")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (1, 2, 3, 4, 5))
@pytest.mark.parametrize("which", ["huge", "tiny"])
def test_gather_extreme_distances(yi, which, kind):
    """squared distances next to the largest finite float and +inf; subnormal and zero ones (and radii whose bits
    leave the bounded walk no histogram bin)"""
    if refused_without_experiments(yi, kind):
        return
    from oracle import oracle as O
    pos, qs, radii = extreme_family(which)
    for k in (1, 7, 64):
        for r2 in radii:
            what = f"kind {kind} {which} k={k} r2={r2!r}"
            got, _ = gpu_gather(yi, pos, qs, kind, k, r2)
            assert_same(got, O.photon_gather(pos, qs, k, r2), what)
            Expect(pos, qs, k, r2).check(got, what)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (3, 4))
def test_long_logs(yi, kind):
    """a log of 60 000 entries per request (every photon of the shell family, see there) below log_cap = 65 536: the
    split heap's 16-bit log positions reach past 2^15; and a map larger than the log, which overflows it"""
    from oracle import oracle as O
    for n, over in ((60_000, False), (70_000, True)):
        pos, qs = shell_family(n)
        for k in (7, 64):
            what = f"kind {kind} shell n={n} k={k}"
            got, r = gpu_gather(yi, pos, qs, kind, k, F(1e30), log_cap=65536, want_log=True)
            assert_same(got, O.photon_gather(pos, qs, k, F(1e30)), what)
            Expect(pos, qs, k, F(1e30)).check(got, what)
            assert r["counters"]["log_cap"] == 65536
            if over:
                assert r["counters"]["overflows"] == len(qs) and (r["log_n"] == n).all(), (what, r["log_n"])
            else:
                assert r["counters"]["overflows"] == 0 and (r["log_n"] == n).all(), (what, r["log_n"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (0, 3, 4))
def test_spill_levels_are_used(yi, kind):
    """leaves on level 21: the first descent of many queries stacks 21 far children (test_spill_map_descends_21_levels),
    the last of them in the walk's HBM spill column"""
    pos, qs = spill_map()
    got, r = gpu_gather(yi, pos, qs, kind, 50, F(1e30))
    c = r["counters"]
    assert c["depth"] == 21 and c["pm_stack"] == 22 and c["lds_levels"] == 20 and c["spill"] == 1, c
    assert_same(got, spill_oracle(), f"kind {kind} spill map")
    spill_expect().check(got, f"kind {kind} spill map")


@functools.lru_cache(maxsize=None)
def deep_oracle():
    from oracle import oracle as O
    pos, qs = deep_map()
    return O.photon_gather(pos, qs, 50, F(1e30))


@functools.lru_cache(maxsize=None)
def deep_expect():
    pos, qs = deep_map()
    return Expect(pos, qs, 50, F(1e30))


@pytest.mark.gpu
def test_render_choice(yi, monkeypatch):
    """kind 0 takes the path a render would: the split replay at k = 64, beyond the register walk's k the one-pass
    gather (the bounded walk in experiments builds); the environment's switches apply"""
    pos, qs = make_map("cube", 257), make_queries("cube", 257)
    path = lambda k: check_family(yi, "cube", 257, 96, 0, k, F(1e30))["counters"]["path"]
    assert path(64) == 4
    assert path(65) == (5 if experiments_built() else 1)
    monkeypatch.setenv("YAFARAY_AMD_GATHER_HEAP", "packed")
    assert path(64) == 3
    monkeypatch.setenv("YAFARAY_AMD_GATHER", "single")
    assert path(64) == 1
    monkeypatch.delenv("YAFARAY_AMD_GATHER")
    monkeypatch.delenv("YAFARAY_AMD_GATHER_HEAP")
    monkeypatch.setenv("YAFARAY_AMD_GATHER_LOG", "8")
    r = check_family(yi, "cube", 257, 96, 0, 7, F(1e30))
    assert r["counters"]["log_cap"] == 8 and r["counters"]["overflows"] > 0 and r["counters"]["path"] == 4


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (1, 3, 4, 6, 8))
def test_photon_order_leaves(yi, monkeypatch, kind):
    """YAFARAY_AMD_PKD_ORDER=photon: leaves index the photons directly instead of the kd-order copies"""
    monkeypatch.setenv("YAFARAY_AMD_PKD_ORDER", "photon")
    for shape in ("cube", "dup4", "lattice"):
        if kind < 6:
            r = check_family(yi, shape, 257, 96, kind, 7, F(1e30))
        else:
            r = check_nearest_family(yi, shape, 257, kind, F(1e30))
        assert r["counters"]["kd_order"] == 0
    monkeypatch.delenv("YAFARAY_AMD_PKD_ORDER")
    assert check_family(yi, "cube", 257, 96, 1, 7, F(1e30))["counters"]["kd_order"] == 1


def check_nearest_family(yi, shape, n, kind, r2, m=192, **kw):
    from oracle import oracle as O
    pos, qs = make_map(shape, n), make_queries(shape, n, m)
    dirs, ns = unit_dirs(n, 5), unit_dirs(len(qs), 6)
    what = f"kind {kind} {shape} n={n} m={m} r2={r2!r} {kw}"
    r = yi.query_photons(pos, qs, kind, radius2=r2, dirs=dirs, normals=ns, **kw)
    exp = nearest_expect(pos, dirs, qs, ns, r2)
    want = O.photon_nearest(pos, dirs, qs, ns, r2)
    assert np.array_equal(r["nearest"], want), f"{what}: differs from findNearest at {np.nonzero(r['nearest'] != want)[0][:8]}"
    check_nearest(exp, r["nearest"], what)
    if kind == 7:
        raw = r["grid_raw"]
        for q, (best, who) in enumerate(exp):
            if raw[q] == -2:
                # the grid's own answer: a tie only where brute force shows one (or no grid was built)
                assert not r["counters"]["grid"] or len(who) > 1, f"{what}: query {q}: -2 without a tie"
            else:
                assert raw[q] == want[q], f"{what}: query {q}: the grid answered {raw[q]}"
        assert r["counters"]["grid_ties"] == int((raw == -2).sum())
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (6, 7, 8))
@pytest.mark.parametrize("shape", SHAPES)
def test_nearest(yi, shape, kind):
    for n in (1, 2, 3, 257, 5000):
        for r2 in radii_for(make_map(shape, n), make_queries(shape, n), 1):
            check_nearest_family(yi, shape, n, kind, r2)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", (6, 7, 8))
def test_nearest_query_counts(yi, kind):
    """m = 1, 63, 64, 65 (below, at and above a wave; one workgroup of 128 lanes) and 1100: the probe launches two
    workgroups, 256 lanes, so every lane serves four or five points"""
    for shape, n, r2 in (("cube", 5000, F(0.01)), ("lattice", 257, F(4.0))):
        for m in (1, 63, 64, 65, 1100):
            check_nearest_family(yi, shape, n, kind, r2, m=m)


@pytest.mark.gpu
def test_nearest_grid_is_used_and_ties_fall_back(yi):
    """the lattice and the duplicated map tie at the nearest distance: the grid says so (-2) and the kd search settles
    it; on the generic map the grid answers every query itself"""
    r = check_nearest_family(yi, "cube", 5000, 7, F(0.01))
    assert r["counters"]["grid"] == 1 and r["counters"]["grid_ties"] == 0
    for shape in ("lattice", "dup4"):
        r = check_nearest_family(yi, shape, 257, 7, F(4.0))
        assert r["counters"]["grid"] == 1 and r["counters"]["grid_ties"] > 0


@pytest.mark.gpu
def test_nearest_lds_stack_levels(yi):
    """pkNearestLds with as many LDS levels as the tree's deepest level (every far child of a path fits) and with
    the render's depth + 1"""
    for shape, n in (("cube", 257), ("cube", 5000), ("line", 257), ("dup4", 5000)):
        depth = yi.query_photons(make_map(shape, n), make_queries(shape, n, 1), 1)["counters"]["depth"]
        for levels in (depth, depth + 1):
            r = check_nearest_family(yi, shape, n, 8, F(1e30), log_cap=levels)
            assert r["counters"]["lds_levels"] == levels


@pytest.mark.gpu
def test_bounded_walk_or_its_refusal(yi):
    pos, qs = make_map("cube", 257), make_queries("cube", 257)
    if experiments_built():
        for k in (1, 7, 64, 65, 100):
            for shape, n in (("cube", 5000), ("lattice", 257), ("octaves", 5000)):
                for r2 in radii_for(make_map(shape, n), make_queries(shape, n), k):
                    check_family(yi, shape, n, 96, 5, k, r2)
    else:
        with pytest.raises(RuntimeError, match="experiments builds only"):
            yi.query_photons(pos, qs, 5, k=7)


@pytest.mark.gpu
def test_bad_arguments_launch_nothing(yi):
    pos, qs = make_map("cube", 257), make_queries("cube", 257)
    max_seg = yi.query_photons(pos, qs[:1], 1)["counters"]["max_seg"]
    for kw, text in ((dict(kind=1, k=0), "k must be at least 1"), (dict(kind=9, k=1), "kind"), (dict(kind=-1, k=1), "kind"),
                     (dict(kind=1, k=1, n_seg=0), "n_seg"), (dict(kind=1, k=1, n_seg=max_seg + 1), "n_seg"),
                     (dict(kind=3, k=7, log_cap=9), "even"), (dict(kind=3, k=7, log_cap=6), "below k"),
                     (dict(kind=3, k=65), "k <= 64"), (dict(kind=4, k=65), "k <= 64"), (dict(kind=6), "bad arrays")):
        kind = kw.pop("kind")
        with pytest.raises(RuntimeError, match=text):
            yi.query_photons(pos, qs, kind, **kw)
    with pytest.raises(RuntimeError, match="at least one photon"):
        yi.query_photons(np.zeros((0, 3), F), qs, 1, k=1)
    # the interface still serves queries
    check_family(yi, "cube", 257, 96, 1, 7, F(1e30))
