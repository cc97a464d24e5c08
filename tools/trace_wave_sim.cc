// CPU wave model of k_trace's BVH4 loop over the Cornell box: the interleaved loop (traverse4: a hit leaf's
// triangles are tested inside the visit) against the deferred one (traverse4Defer: a visit records its hit leaves
// in a per-lane list of `cap` leaf entries, the triangles are tested in one dense loop once the lane's traversal
// has ended or its list has no room for the four leaves of another visit).  Host only; the tree is the
// project's own (bvh.cc, buildBvh(in, 1, 1) as host.cc builds LDS-resident scenes).
//
//   g++ -O2 -std=c++17 -o trace_wave_sim tools/trace_wave_sim.cc libyafaray_amd/csrc/bvh.cc -pthread && ./trace_wave_sim
//
// Rays: a 48 x 27 pixel grid of the C2 camera, 64 samples per pixel = one wave of 64 consecutive queue entries;
// every hit spawns a cosine-distributed bounce ray and a shadow ray towards a point of the area light; the
// queues are compacted between iterations (closest: rays that hit; shadow: one per hit), as the renderer's are.
// A wave runs its lanes in lockstep: a loop's trip count is the largest count of any lane.  Instruction costs
// per wave (DESIGN §5 "C2 k_trace instruction budget"): setup 91, visit 84 + the order network (60 closest, 30
// any-hit), triangle test 97; the deferred loop adds kAppend per visit (four list stores and the slot
// arithmetic) and kTrip per triangle trip (the leaf cursor).
// The flat scan (traverseFlat) has no box traversal: every ray tests the L leaf boxes of the scene's leaf table
// (bvh.cc buildFlatTable) against [box_t0, slack(tmax)] at kFlatBox VALU each, in a wave-uniform loop, then its
// pending triangles lowest slot first (kTri per trip; no leaf cursor).  The last line prints the lists' box
// traversal per wave on the whole mix and the leaf count at which kFlatBox L reaches it (bvh.h kFlatMaxLeaves).
// The model asserts that all loops return the same (t, primitive) / occlusion for every ray.
#include "../libyafaray_amd/csrc/bvh.h"

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <vector>

using namespace yafamd;

constexpr int kSetup = 91, kVisit = 84, kOrderClosest = 60, kOrderAny = 30, kTri = 97, kAppend = 12, kTrip = 6;
constexpr int kFlatBox = 19;   // 6 FMA, 6 min / max, max3 + max, min3 + min, compare, select + OR (from reading the slab test)
constexpr int kRoom = 4;   // free entries a visit needs (kernels.hip kDeferRoom)

static int asInt(float f) { int i; std::memcpy(&i, &f, 4); return i; }

struct V { float x, y, z; };
static V operator+(V a, V b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
static V operator-(V a, V b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
static V operator*(V a, float s) { return {a.x * s, a.y * s, a.z * s}; }
static float dot(V a, V b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
static V cross(V a, V b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
static V unit(V a) { return a * (1.f / std::sqrt(dot(a, a))); }

struct Ray { V o, d; float tmin, tmax; };

// primitive_triangle.cc:44-71 on the packed record (v0, e1, e2, eps)
static float triTest(const float *r, const Ray &ray)
{
	const V v0{r[0], r[1], r[2]}, e1{r[4], r[5], r[6]}, e2{r[8], r[9], r[10]};
	const float eps = r[3];
	const V p = cross(ray.d, e2);
	const float det = dot(e1, p);
	if(det > -eps && det < eps) return -1.f;
	const float inv = 1.f / det;
	const V tv = ray.o - v0;
	const float u = dot(tv, p) * inv;
	if(u < 0.f || u > 1.f) return -1.f;
	const V q = cross(tv, e1);
	const float v = dot(ray.d, q) * inv;
	if(v < 0.f || u + v > 1.f) return -1.f;
	const float t = dot(e2, q) * inv;
	return t < eps ? -1.f : t;
}

struct Scene
{
	std::vector<float> verts;
	std::vector<int> tris;
	BvhOutput bvh;
};

static void quad(Scene &s, V a, V b, V c, V d)
{
	const int v0 = (int)s.verts.size() / 3;
	for(V p : {a, b, c, d}) { s.verts.push_back(p.x); s.verts.push_back(p.y); s.verts.push_back(p.z); }
	for(int i : {0, 1, 2, 0, 2, 3}) s.tris.push_back(v0 + i);
}

static void box(Scene &s, float cx, float cy, float sx, float sy, float h, float deg)
{
	const float a = deg * 3.14159265358979f / 180.f, ca = std::cos(a), sa = std::sin(a);
	const int v0 = (int)s.verts.size() / 3;
	const float ux[4] = {-sx, sx, sx, -sx}, uy[4] = {-sy, -sy, sy, sy};
	for(float dz : {0.f, h})
		for(int k = 0; k < 4; ++k) { s.verts.push_back(cx + ux[k] * ca - uy[k] * sa); s.verts.push_back(cy + ux[k] * sa + uy[k] * ca); s.verts.push_back(dz); }
	const int t[36] = {0, 2, 1, 0, 3, 2, 4, 5, 6, 4, 6, 7, 0, 1, 5, 0, 5, 4, 1, 2, 6, 1, 6, 5, 2, 3, 7, 2, 7, 6, 3, 0, 4, 3, 4, 7};
	for(int i : t) s.tris.push_back(v0 + i);
}

// scenes.cornell
static Scene cornell()
{
	Scene s;
	quad(s, {-1, -1, 0}, {1, -1, 0}, {1, 1, 0}, {-1, 1, 0});
	quad(s, {-1, -1, 2}, {-1, 1, 2}, {1, 1, 2}, {1, -1, 2});
	quad(s, {-1, 1, 0}, {1, 1, 0}, {1, 1, 2}, {-1, 1, 2});
	quad(s, {-1, -1, 0}, {-1, 1, 0}, {-1, 1, 2}, {-1, -1, 2});
	quad(s, {1, -1, 0}, {1, -1, 2}, {1, 1, 2}, {1, 1, 0});
	box(s, 0.35f, -0.25f, 0.3f, 0.3f, 0.6f, -17.f);
	box(s, -0.35f, 0.35f, 0.3f, 0.3f, 1.2f, 17.f);
	BvhInput in{s.verts.data(), s.tris.data(), (int)s.tris.size() / 3};
	s.bvh = buildBvh(in, 1, 1);
	return s;
}

// What one ray does: per round (a flush of the deferred loop; the interleaved loop has one round per visit)
// the visits and the triangle tests of the round
struct Round { int visits, tests; };
struct Trace
{
	std::vector<Round> rounds;
	float t = 0.f;
	int prim = -1, visits = 0, tests = 0;
};

// cap == 0: the interleaved loop; cap >= kRoom: the deferred loop with `cap` leaf entries per lane
static Trace traverse(const BvhOutput &b, const Ray &r, bool any, int cap)
{
	Trace T;
	float t_best = r.tmax;
	int prim_best = -1;
	std::vector<int> stack;
	std::vector<std::pair<int, int>> pending;   // (first slot, count)
	const float t0 = any ? -1e-3f : r.tmin - 1e-3f * (1.f + std::fabs(r.tmin));
	int node = 0;
	bool done = false;
	auto testLeaf = [&](int start, int count, int &tests) {
		for(int q = start; q < start + count && !done; ++q)
		{
			++tests;
			const float *rec = &b.tris[12 * (size_t)q];
			const float t = triTest(rec, r);
			if(t == -1.f) continue;
			const int prim = asInt(rec[7]);
			if(any) { if(t < r.tmax && t >= 0.f) { t_best = t; prim_best = prim; done = true; } }
			else if(t >= r.tmin && (t < t_best || (t == t_best && prim_best >= 0 && prim < prim_best))) { t_best = t; prim_best = prim; }
		}
	};
	while(!done)
	{
		Round R{0, 0};
		// phase 1 (interleaved: exactly one visit, its leaves tested at once)
		while(node >= 0 && (cap == 0 ? R.visits == 0 : (int)pending.size() + kRoom <= cap))
		{
			++R.visits;
			const float *o = &b.nodes[32 * (size_t)node];
			const float slack = t_best < 3.0e38f ? t_best * 1.0000005f + 1e-6f : 3.4e38f;
			std::vector<std::pair<float, int>> inner;
			for(int k = 0; k < 4 && !done; ++k)
			{
				float lo = t0, hi = slack;
				const float od[3] = {r.o.x, r.o.y, r.o.z}, dd[3] = {r.d.x, r.d.y, r.d.z};
				for(int a = 0; a < 3; ++a)
				{
					const float d = std::fabs(dd[a]) < 1e-20f ? std::copysign(1e-20f, dd[a]) : dd[a];
					const float ta = (o[8 * a + k] - od[a]) / d, tb = (o[8 * a + 4 + k] - od[a]) / d;
					lo = std::max(lo, std::min(ta, tb));
					hi = std::min(hi, std::max(ta, tb));
				}
				if(!(lo <= hi)) continue;
				const int c = asInt(o[24 + k]), cnt = asInt(o[28 + k]);
				if(c >= 0) { inner.push_back({lo, c}); continue; }
				if(cnt == 0) continue;
				if(cap == 0) testLeaf(~c, cnt, R.tests);
				else pending.push_back({~c, cnt});
			}
			if(done) break;
			if(!any) std::stable_sort(inner.begin(), inner.end(), [](auto &x, auto &y) { return x.first < y.first; });
			for(int k = (int)inner.size() - 1; k >= 1; --k) stack.push_back(inner[k].second);
			if(!inner.empty()) node = inner[0].second;
			else if(!stack.empty()) { node = stack.back(); stack.pop_back(); }
			else node = -1;
		}
		// phase 2: the pending leaves, last recorded first
		while(!pending.empty() && !done)
		{
			const auto [start, count] = pending.back();
			pending.pop_back();
			testLeaf(start, count, R.tests);
		}
		T.rounds.push_back(R);
		T.visits += R.visits;
		T.tests += R.tests;
		if(node < 0) break;
	}
	T.t = t_best;
	T.prim = prim_best;
	return T;
}

// The flat scan: one round, no visits
static Trace traverseFlat(const BvhOutput &b, const FlatTable &ft, const Ray &r, bool any)
{
	Trace T;
	float t_best = r.tmax;
	int prim_best = -1;
	const float t0 = any ? -1e-3f : r.tmin - 1e-3f * (1.f + std::fabs(r.tmin));
	const float slack = r.tmax < 3.0e38f ? r.tmax * 1.0000005f + 1e-6f : 3.4e38f;
	uint64_t m = 0;
	const float od[3] = {r.o.x, r.o.y, r.o.z}, dd[3] = {r.d.x, r.d.y, r.d.z};
	for(int i = 0; i < ft.n; ++i)
	{
		const FlatLeaf &l = ft.rec[i];
		float lo = t0, hi = slack;
		for(int a = 0; a < 3; ++a)
		{
			const float d = std::fabs(dd[a]) < 1e-20f ? std::copysign(1e-20f, dd[a]) : dd[a];
			const float ta = (l.lo[a] - od[a]) / d, tb = (l.hi[a] - od[a]) / d;
			lo = std::max(lo, std::min(ta, tb));
			hi = std::min(hi, std::max(ta, tb));
		}
		if(lo <= hi) m |= ((uint64_t)l.bits_hi << 32) | l.bits_lo;
	}
	Round R{0, 0};
	for(int q = 0; q < 64; ++q)
	{
		if(!((m >> q) & 1)) continue;
		++R.tests;
		const float *rec = &b.tris[12 * (size_t)q];
		const float t = triTest(rec, r);
		if(t == -1.f) continue;
		const int prim = asInt(rec[7]);
		if(any) { if(t < r.tmax && t >= 0.f) { t_best = t; prim_best = prim; break; } }
		else if(t >= r.tmin && (t < t_best || (t == t_best && prim_best >= 0 && prim < prim_best))) { t_best = t; prim_best = prim; }
	}
	T.rounds.push_back(R);
	T.tests = R.tests;
	T.t = t_best;
	T.prim = prim_best;
	return T;
}

// VALU wave-instructions of one wave of rays and the trips of its triangle loops
struct WaveCost { double valu = 0, trips = 0, iters = 0; };
static WaveCost waveCost(const std::vector<Trace> &lanes, bool any, bool deferred, int flat_leaves = 0)
{
	WaveCost c;
	c.valu = kSetup;
	if(flat_leaves)
	{
		int tt = 0;
		for(const Trace &t : lanes) tt = std::max(tt, t.tests);
		c.trips = tt;
		c.valu += (double)flat_leaves * kFlatBox + (double)tt * kTri;
		return c;
	}
	const int order = any ? kOrderAny : kOrderClosest;
	size_t rounds = 0;
	for(const Trace &t : lanes) rounds = std::max(rounds, t.rounds.size());
	for(size_t r = 0; r < rounds; ++r)
	{
		int v = 0, tt = 0;
		for(const Trace &t : lanes)
			if(r < t.rounds.size()) { v = std::max(v, t.rounds[r].visits); tt = std::max(tt, t.rounds[r].tests); }
		c.iters += v;
		c.trips += tt;
		c.valu += (double)v * (kVisit + order + (deferred ? kAppend : 0)) + (double)tt * (kTri + (deferred ? kTrip : 0));
	}
	return c;
}

int main()
{
	const Scene S = cornell();
	const BvhOutput &b = S.bvh;
	const FlatTable ft = buildFlatTable(b.nodes.data(), b.n_nodes);
	std::printf("Cornell: %d triangles, %d BVH4 nodes, largest leaf %d, %d leaves (%d / %d / %d by mask word)\n", (int)S.tris.size() / 3, b.n_nodes,
	            b.max_leaf, ft.n, ft.n_lo, ft.n_mid - ft.n_lo, ft.n - ft.n_mid);
	std::mt19937 rng(11);
	std::uniform_real_distribution<float> U(0.f, 1.f);
	auto normalOf = [&](int prim) {
		const int *t = &S.tris[3 * prim];
		auto P = [&](int v) { return V{S.verts[3 * v], S.verts[3 * v + 1], S.verts[3 * v + 2]}; };
		return unit(cross(P(t[1]) - P(t[0]), P(t[2]) - P(t[0])));
	};
	// iteration 0: camera rays (from (0, -3.9, 1) towards y, focal 1.4, 16:9), 64 jittered samples per pixel
	const int W = 48, H = 27;
	std::vector<Ray> closest, shadow;
	for(int y = 0; y < H; ++y)
		for(int x = 0; x < W; ++x)
			for(int s = 0; s < 64; ++s)
			{
				const float u = ((x + U(rng)) / W - 0.5f), v = ((y + U(rng)) / H - 0.5f) * (float)H / W;
				closest.push_back({{0.f, -3.9f, 1.f}, unit({u, 1.4f, -v}), 0.f, 3.4e38f});
			}
	const std::vector<int> caps = {0, 4, 6, 8, 12, 16};
	std::vector<double> total(caps.size(), 0.0);
	double total_flat = 0, lists_box = 0, lists_waves = 0;   // lists_box: the cap-8 lists' box traversal (visits only)
	std::printf("%-12s %6s %7s %7s |", "launch", "waves", "visits", "tests");
	for(int cap : caps)
	{
		if(cap) std::printf("  cap %-2d valu trips |", cap);
		else std::printf("  interleaved trips |");
	}
	std::printf("  flat   valu trips |\n");
	for(int it = 0; it < 4; ++it)
	{
		for(int kind = 0; kind < 2; ++kind)
		{
			const bool any = kind == 1;
			const std::vector<Ray> &Q = any ? shadow : closest;
			if(Q.empty()) continue;
			std::vector<std::vector<Trace>> tr(caps.size());
			for(size_t c = 0; c < caps.size(); ++c)
				for(const Ray &r : Q) tr[c].push_back(traverse(b, r, any, caps[c]));
			// the deferred order returns what the interleaved one does
			for(size_t c = 1; c < caps.size(); ++c)
				for(size_t i = 0; i < Q.size(); ++i)
				{
					const Trace &a = tr[0][i], &d = tr[c][i];
					const bool same = any ? ((a.prim >= 0) == (d.prim >= 0)) : (a.prim == d.prim && (a.prim < 0 || a.t == d.t));
					if(!same) { std::printf("MISMATCH it %d kind %d ray %zu cap %d: (%g %d) vs (%g %d)\n", it, kind, i, caps[c], a.t, a.prim, d.t, d.prim); return 1; }
				}
			const size_t waves = (Q.size() + 63) / 64;
			double v0 = 0, t0 = 0;
			for(const Trace &t : tr[0]) { v0 += t.visits; t0 += t.tests; }
			std::printf("%d %-10s %6zu %7.2f %7.2f |", it, any ? "shadow" : "closest", waves, v0 / Q.size(), t0 / Q.size());
			for(size_t c = 0; c < caps.size(); ++c)
			{
				double valu = 0, trips = 0;
				for(size_t w = 0; w < waves; ++w)
				{
					const std::vector<Trace> lanes(tr[c].begin() + 64 * w, tr[c].begin() + std::min(Q.size(), 64 * (w + 1)));
					const WaveCost k = waveCost(lanes, any, caps[c] != 0);
					valu += k.valu;
					trips += k.trips;
				}
				total[c] += valu;
				std::printf("  %11.0f %5.1f |", valu / waves, trips / waves);
				if(caps[c] == 8)
					for(size_t w = 0; w < waves; ++w)
					{
						const std::vector<Trace> lanes(tr[c].begin() + 64 * w, tr[c].begin() + std::min(Q.size(), 64 * (w + 1)));
						lists_box += waveCost(lanes, any, true).iters * (kVisit + (any ? kOrderAny : kOrderClosest) + kAppend);
						lists_waves += 1;
					}
			}
			{
				std::vector<Trace> fl;
				for(size_t i = 0; i < Q.size(); ++i)
				{
					fl.push_back(traverseFlat(b, ft, Q[i], any));
					const Trace &a = tr[0][i], &d = fl.back();
					const bool same = any ? ((a.prim >= 0) == (d.prim >= 0)) : (a.prim == d.prim && (a.prim < 0 || a.t == d.t));
					if(!same) { std::printf("MISMATCH it %d kind %d ray %zu flat: (%g %d) vs (%g %d)\n", it, kind, i, a.t, a.prim, d.t, d.prim); return 1; }
				}
				double valu = 0, trips = 0;
				for(size_t w = 0; w < waves; ++w)
				{
					const std::vector<Trace> lanes(fl.begin() + 64 * w, fl.begin() + std::min(Q.size(), 64 * (w + 1)));
					const WaveCost k = waveCost(lanes, any, false, ft.n);
					valu += k.valu;
					trips += k.trips;
				}
				total_flat += valu;
				std::printf("  %11.0f %5.1f |", valu / waves, trips / waves);
			}
			std::printf("\n");
		}
		// the next iteration's queues: every hit bounces (cosine-distributed) and casts one shadow ray
		std::vector<Ray> nc, ns;
		for(const Ray &r : closest)
		{
			const Trace t = traverse(b, r, false, 0);
			if(t.prim < 0) continue;
			V n = normalOf(t.prim);
			if(dot(n, r.d) > 0.f) n = n * -1.f;
			const V p = r.o + r.d * t.t;
			const float u1 = U(rng), u2 = U(rng), rad = std::sqrt(u1), phi = 6.2831853f * u2;
			const V a = std::fabs(n.x) > 0.5f ? V{0, 1, 0} : V{1, 0, 0};
			const V tx = unit(cross(n, a)), ty = cross(n, tx);
			nc.push_back({p, unit(tx * (rad * std::cos(phi)) + ty * (rad * std::sin(phi)) + n * std::sqrt(1.f - u1)), 5e-5f, 3.4e38f});
			const V l{-0.25f + 0.5f * U(rng), -0.25f + 0.5f * U(rng), 1.98f};
			const V dl = l - p;
			const float dist = std::sqrt(dot(dl, dl));
			if(dot(dl, n) > 0.f) ns.push_back({p + unit(dl) * 5e-5f, unit(dl), 0.f, dist - 1e-4f});
		}
		closest.swap(nc);
		shadow.swap(ns);
	}
	std::printf("whole mix (VALU summed over all waves, interleaved = 1):");
	for(size_t c = 0; c < caps.size(); ++c) std::printf("  %s%d %.3f", caps[c] ? "cap " : "interleaved ", caps[c], total[c] / total[0]);
	std::printf("  flat %.3f\n", total_flat / total[0]);
	std::printf("lists (cap 8): box traversal %.0f VALU per wave on the whole mix = %d VALU x %.1f leaf boxes\n", lists_box / lists_waves, kFlatBox,
	            lists_box / lists_waves / kFlatBox);
	return 0;
}
