// BVH traversal of the MI355X path-tracing core (device code only): the ray / box / triangle steps and the
// loops built from them.  The kernels that run the loops (k_trace, k_path, k_nee, the photon and final-gather
// kernels, the render layers) and their launch code live in kernels.hip and layers.hip.
//
// The loops (traverse2, traverse4, traverse4Defer, traverseFlat, traceRefill4, traceRefill8, traceLaneRays) share
// these steps, each defined once here:
//
//   rayPrep      the ray's inverse direction (with the 1e-20 clamp), o / d, the near / far plane selectors
//                and the padded entry distance box_t0
//   slackOf      the box culling distance for the closest hit so far
//   node4 / ldsF4, slab4   a BVH4 node's planes for the ray, one child's slab distances
//   triTest      the exact triangle test
//   HIT_CLOSER / HIT_ANY / HIT_ANY_TS   hit acceptance: closest (ties -> lower primitive index), any-hit
//                and transparent-shadow
//   sort4 / sort8   the child-order networks
//   stackPush / stackPop   the per-lane stack: LDS levels, then the spill column
//
// The loops keep what differs between them (when the slack is recomputed, how empty leaves are skipped,
// where the lane's stack column comes from) and the steps whose shared form changed the generated code:
// the child / count / leaf bookkeeping of a BVH4 visit, the per-lane leaf span, the pushes after the
// network and the refill loops' queue fetch and write-back (profiles/trace_refactor.md).  Every ray of
// every loop runs the same visits, culling, leaf order and exits as traverse4 (traverse4Defer: a superset
// of the visits; traverseFlat: every leaf box, no inner visit), so hits are identical.
//
// Compiled with -ffp-contract=off: every float expression keeps the reference's order.
#pragma once

#include <hip/hip_runtime.h>
#include "bvh.h"
#include "devmath.h"
#include "devscene.h"

namespace yafamd
{

#ifndef YAF_TRACE_BLOCK
#define YAF_TRACE_BLOCK 128
#endif
constexpr int kTraceBlock = YAF_TRACE_BLOCK;

__device__ __forceinline__ V3 xyz(const float4 &a) { return v3(a.x, a.y, a.z); }

// ---------------------------------------------------------------------------------------------
// Queue ray accessors
// ---------------------------------------------------------------------------------------------

// 12-byte records (one dwordx3 per lane, 4-byte aligned): the pending throughput, whose fourth
// component was never read
struct F3
{
	float x, y, z;
};

// Closest-ray queue entry i (DevQueues::ray_o / ray_d: 12-B records, 24 B per ray instead of 32):
// false when the entry carries no ray this iteration (NaN direction x).  tmin / tmax (< 0:
// infinite) come from ray_tt in a pass's first iteration when its rays carry their own (spawned rays;
// camera rays with clip planes), else (Q.tmin_dflt, infinite): camera rays 0, k_shade's bounces
// ray_min_dist.
// -DYAF_NT_RAYLOAD=1: the ray streams of k_trace are loaded / stored non-temporally (streaming
// lines evicted first: the node working set of a BVH in global memory keeps more of the L2)
#ifndef YAF_NT_RAYLOAD
#define YAF_NT_RAYLOAD 0
#endif
typedef float f32x4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ F3 rayLd3(const float *p, uint32_t i)
{
#if YAF_NT_RAYLOAD
	const float *q = p + 3 * (size_t)i;
	return F3{__builtin_nontemporal_load(q), __builtin_nontemporal_load(q + 1), __builtin_nontemporal_load(q + 2)};
#else
	return reinterpret_cast<const F3 *>(p)[i];
#endif
}
__device__ __forceinline__ float4 rayLd4(const float4 *p)
{
#if YAF_NT_RAYLOAD
	const f32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const f32x4_t *>(p));
	return make_float4(v.x, v.y, v.z, v.w);
#else
	return *p;
#endif
}
template<class T>
__device__ __forceinline__ void raySt(T *p, T v)
{
#if YAF_NT_RAYLOAD
	__builtin_nontemporal_store(v, p);
#else
	*p = v;
#endif
}

__device__ __forceinline__ bool loadQRay(const DevQueues &Q, uint32_t i, V3 &o, V3 &d, float &tmin, float &tmax_w)
{
	// (both records loaded before the test: one memory round trip, not two dependent ones)
	const F3 dd = rayLd3(Q.ray_d, i);
	const F3 oo = rayLd3(Q.ray_o, i);
	d = v3(dd.x, dd.y, dd.z);
	o = v3(oo.x, oo.y, oo.z);
	if(dd.x != dd.x) return false;
	if(Q.ray_tt)
	{
		const float2 tt = Q.ray_tt[i];
		tmin = tt.x;
		tmax_w = tt.y;
	}
	else
	{
		tmin = Q.tmin_dflt;
		tmax_w = -1.f;
	}
	return true;
}

// ---------------------------------------------------------------------------------------------
// Traversal context and the per-lane stack
// ---------------------------------------------------------------------------------------------
#ifndef YAF_TOP_STRIDE
#define YAF_TOP_STRIDE 9
#endif
constexpr int kTopStride = YAF_TOP_STRIDE;   // float4 per node of the LDS top treelet (8 used + 1 pad)
struct TraceCtx
{
	const float4 *nodes;
	const float4 *tris;
	int *stack;     // LDS, [level * kTraceBlock + lane], levels [0, lds_depth)
	int lds_depth;
	int *spill;     // HBM, [(level - lds_depth) * spill_stride + global lane] (BVH4 deep levels)
	uint32_t spill_stride;
	// the top treelet of a BVH4 in global memory staged in LDS: nodes [0, n_top) at kTopStride float4 each
	// (144 B: a 128-B stride put every node's plane p on the same 4 of the 64 banks, so the 16 lanes of a
	// ds_read_b128 group at different nodes conflicted up to 8-way; 36-dword strides spread 16 nodes
	// over 16 distinct bank quads) (both builders number
	// the wide nodes level by level, so these are the levels every ray starts with)
	const float4 *top = nullptr;
	int n_top = 0;
	uint32_t wave_base = 0;   // threadIdx.x of the wave's lane 0 (scalar; set with the context: waveBase())
};
// threadIdx.x of the wave's first lane, and this lane's threadIdx.x re-derived from it (v_mbcnt, opaque so
// that it is recomputed where used instead of keeping threadIdx.x live — or spilled — across the loops)
__device__ __forceinline__ uint32_t waveBase() { return __builtin_amdgcn_readfirstlane((uint32_t)threadIdx.x) & ~63u; }
__device__ __forceinline__ uint32_t tidFrom(uint32_t wave_base)
{
	uint32_t l;
	asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(l));
	return wave_base + l;
}

// Level `sp` of this lane's traversal stack: C.stack[sp * STRIDE + column] for the LDS levels; with SPILL the
// levels from C.lds_depth on (rare) live in this lane's HBM column (`glane`: the lane's index in the grid).
// Without SPILL the loop's stack bound fits the LDS levels and every access is a plain LDS access (with a
// possible spill the compiler merges both address spaces into flat accesses, whose pops wait for every
// outstanding vector-memory operation).
// REMAT: the column is the wave's first thread (scalar) plus the lane id (v_mbcnt), re-derived at every
// push / pop — opaque, so not hoisted: at the 64-VGPR budget a loop-invariant column address was spilled
// and reloaded from scratch at every push (a vector-memory wait per push).  Otherwise the column is `lane`,
// threadIdx.x read once by the loop (with REMAT `lane` is not used).  Each loop's choice was a
// register-budget decision.
template<bool REMAT>
__device__ __forceinline__ int stackColumn(const TraceCtx &C, int lane)
{
	if constexpr(REMAT) return (int)tidFrom(C.wave_base);
	else return lane;
}
template<int STRIDE, bool SPILL, bool REMAT>
__device__ __forceinline__ void stackPush(const TraceCtx &C, int sp, int lane, uint32_t glane, int v)
{
	if(!SPILL || sp < C.lds_depth) C.stack[sp * STRIDE + stackColumn<REMAT>(C, lane)] = v;
	else if(SPILL) C.spill[(uint32_t)(sp - C.lds_depth) * C.spill_stride + glane] = v;
}
template<int STRIDE, bool SPILL, bool REMAT>
__device__ __forceinline__ int stackPop(const TraceCtx &C, int sp, int lane, uint32_t glane)
{
	return (!SPILL || sp < C.lds_depth) ? C.stack[sp * STRIDE + stackColumn<REMAT>(C, lane)]
	                                    : C.spill[(uint32_t)(sp - C.lds_depth) * C.spill_stride + glane];
}

// ---------------------------------------------------------------------------------------------
// Ray setup, box and triangle tests, hit acceptance
// ---------------------------------------------------------------------------------------------

// Correctly rounded 1/x: v_rcp_f32 + one FMA Newton step, which tools/rcp_check.hip
// verified exhaustively on gfx950 to equal the IEEE quotient for every float with
// 2^-125 <= |x| <= 2^125 (other magnitudes, zero, inf and NaN take the IEEE division).
__device__ __forceinline__ float rcpExact(float x)
{
	const float ax = fabsf(x);
	if(ax >= 0x1p-125f && ax <= 0x1p125f)
	{
		const float y = __builtin_amdgcn_rcpf(x);
		return __builtin_fmaf(y, __builtin_fmaf(-x, y, 1.f), y);
	}
	return 1.f / x;
}

// Near / far planes of a BVH4 node's boxes for one ray.  By the sign of the inverse direction the
// slab's entry plane is the low bound (1/d >= 0) or the high one for every box, and fma(b, 1/d, -o/d)
// is monotone in b, so max(near distances) / min(far distances) are exactly the values of the
// per-child min / max over both planes — 4 x 6 fewer min / max per visit for six per-lane addresses.
struct SlabSel { int nx, ny, nz; };   // float4 index in the node of the near plane per axis (far: ^ 1)
__device__ __forceinline__ SlabSel slabSel(V3 id) { return SlabSel{id.x >= 0.f ? 0 : 1, id.y >= 0.f ? 2 : 3, id.z >= 0.f ? 4 : 5}; }

// What every box test of one ray needs.  The BVH2 loops test (bound - o) * id (boxPair) and use id and
// box_t0 only; the wide loops test fma(bound, id, -oid): the rounding of o/d is covered by the boxes'
// build-time padding (mag * 1e-5, bvh.cc padBox) as the rounding of (bound - o) is.  box_t0 is the entry
// distance boxes are culled against: any-hit rays start at 0, closest rays at tmin, both padded.
struct RayPrep
{
	V3 id, oid;
	SlabSel sel;
	float box_t0;
};
__device__ __forceinline__ RayPrep rayPrep(V3 o, V3 d, float tmin, bool any)
{
	V3 dd = d;
	if(fabsf(dd.x) < 1e-20f) dd.x = copysignf(1e-20f, dd.x);
	if(fabsf(dd.y) < 1e-20f) dd.y = copysignf(1e-20f, dd.y);
	if(fabsf(dd.z) < 1e-20f) dd.z = copysignf(1e-20f, dd.z);
	RayPrep R;
	R.id = v3(rcpExact(dd.x), rcpExact(dd.y), rcpExact(dd.z));
	R.oid = v3(o.x * R.id.x, o.y * R.id.y, o.z * R.id.z);
	R.sel = slabSel(R.id);
	R.box_t0 = any ? -1e-3f : (tmin - 1e-3f * (1.f + fabsf(tmin)));
	return R;
}

// The box culling distance for a closest hit at t (a relative and an absolute slack: box tests are
// conservative, so culling never drops a hit the exhaustive reference semantics would return)
__device__ __forceinline__ float slackOf(float t) { return (t < 3.0e38f) ? t * 1.0000005f + 1e-6f : 3.4e38f; }

__device__ __forceinline__ void boxPair(const float4 &n0, const float4 &n1, const float4 &n2, V3 o, V3 id,
                                        float t0, float t1, bool &h0, bool &h1, float &tn0, float &tn1)
{
	// child 0
	float ax = (n0.x - o.x) * id.x, bx = (n0.y - o.x) * id.x;
	float ay = (n0.z - o.y) * id.y, by = (n0.w - o.y) * id.y;
	float az = (n2.x - o.z) * id.z, bz = (n2.y - o.z) * id.z;
	float lo = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), t0));
	float hi = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), t1));
	h0 = lo <= hi;
	tn0 = lo;
	ax = (n1.x - o.x) * id.x; bx = (n1.y - o.x) * id.x;
	ay = (n1.z - o.y) * id.y; by = (n1.w - o.y) * id.y;
	az = (n2.z - o.z) * id.z; bz = (n2.w - o.z) * id.z;
	lo = fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fmaxf(fminf(az, bz), t0));
	hi = fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fminf(fmaxf(az, bz), t1));
	h1 = lo <= hi;
	tn1 = lo;
}

// primitive_triangle.cc:44-71.  Returns t or -1.  The reference's arithmetic (correctly rounded
// 1/det, then products) evaluated branch-free: every lane computes the same instruction stream
// and the reference's early returns become one combined predicate (NaN comparisons keep their
// reference outcome).  (The short-circuit form is kept on
// purpose: the compiler turns it into det -> u -> (v, t) early outs; a bitwise predicate that
// computes every term measured k_trace 27.6 -> 35.4 ms per C2 frame.)
__device__ __forceinline__ float triTest(const float4 &a, const float4 &b, const float4 &c, V3 o, V3 d)
{
	const V3 v0 = xyz(a), e1 = xyz(b), e2 = xyz(c);
	const float eps = a.w;
	const V3 pvec = cross(d, e2);
	const float det = dot(e1, pvec);
	const float inv_det = rcpExact(det);
	const V3 tvec = o - v0;
	const float u = dot(tvec, pvec) * inv_det;
	const V3 qvec = cross(tvec, e1);
	const float v = dot(d, qvec) * inv_det;
	const float t = dot(e2, qvec) * inv_det;
	const bool miss = (det > -eps && det < eps) || (u < 0.f || u > 1.f) || (v < 0.f) || ((u + v) > 1.f) || (t < eps);
	return miss ? -1.f : t;
}

// Transparent-shadow hit list of one shadow ray (accelerator_kdtree.cc:1001-1023): an opaque
// surface shadows; each transparent one is recorded until `cap` (= shadowDepth) are recorded, the
// next one shadows.  A BVH holds every triangle once, so the reference's `filtered` set (one
// factor per primitive) needs no lookup.
struct TsList
{
	float2 *hit;
	int n, cap;
	const float4 *prim_ng;
	const DevMaterial *mats;
};

__device__ __forceinline__ bool tsShadows(TsList &L, float t, int prim)
{
	const int mat = __float_as_int(L.prim_ng[prim].w);
	if(!(L.mats[mat].sd_flags & SD_TRANSPARENT)) return true;
	if(L.n >= L.cap) return true;
	L.hit[L.n] = make_float2(t, __int_as_float(prim));
	++L.n;
	return false;
}

// Hit acceptance: a triangle hit at t (triTest's, not -1) of primitive `prim` against the ray's result so far.
//   HIT_CLOSER: t in [tmin, t_best), equal t -> the lower primitive index; the ray goes on with the nearer hit
//   HIT_ANY:    t in [0, tmax): the ray is occluded and ends
//   HIT_ANY_TS: intersectTs: t in [tmin, t_max) of the moved ray (tmin kept, accelerator.cc:82-85) on a
//               surface that shadows (tsShadows records the transparent ones): the ray ends
// Expressions, not functions, on purpose: a predicate function is optimised on its own before it is inlined
// and reaches the loop as a value (a result register, or a predicate computed in full), where the loops
// branch on the terms one by one — every function form tried (by value, by reference, with the stores, with
// a result code) changed k_trace's code and its registers at the 64-VGPR budget.
#define HIT_CLOSER(t, prim, tmin, t_best, prim_best) \
	((t) >= (tmin) && ((t) < (t_best) || ((t) == (t_best) && (prim_best) >= 0 && (prim) < (prim_best))))
#define HIT_ANY(t, tmax) ((t) < (tmax) && (t) >= 0.f)
#define HIT_ANY_TS(t, prim, tmin, tmax, ts) ((t) < (tmax) && (t) >= (tmin) && tsShadows(*(ts), t, prim))

// per-visit statistics of the traversal (node visits, triangle tests); -DYAF_TRACE_NOSTATS drops them
#ifdef YAF_TRACE_NOSTATS
#define TRACE_STAT(x) do {} while(0)
#else
#define TRACE_STAT(x) x
#endif

// ---------------------------------------------------------------------------------------------
// BVH2
// ---------------------------------------------------------------------------------------------

// Closest hit with t in [tmin, tmax) (ties -> lower primitive index), or any hit with t in
// [0, tmax).  Box tests are conservative (boxes padded at build time + a relative slack), so
// culling never drops a hit the exhaustive reference semantics would return.
template<bool ANY, bool TS = false, bool STATS = true>
__device__ bool traverse2(const TraceCtx &C, V3 o, V3 d, float tmin, float tmax, float &t_best, int &prim_best,
                          uint32_t &visits, uint32_t &tests, TsList *ts = nullptr)
{
	const int lane = threadIdx.x;
	const RayPrep R = rayPrep(o, d, tmin, ANY);
	t_best = tmax;
	prim_best = -1;
	int sp = 0;
	int node = 0;
	for(;;)
	{
		if(STATS) TRACE_STAT(++visits);
		const float4 *np = C.nodes + 4 * node;
		const float4 n0 = np[0], n1 = np[1], n2 = np[2], n3 = np[3];
		const float slack_t = slackOf(t_best);
		bool h0, h1;
		float tn0, tn1;
		boxPair(n0, n1, n2, o, R.id, R.box_t0, slack_t, h0, h1, tn0, tn1);
		const int c0 = __float_as_int(n3.x), c1 = __float_as_int(n3.y);
		const int k0 = __float_as_int(n3.z), k1 = __float_as_int(n3.w);
		int next = -1;
		// leaves are tested right away; inner children are descended nearest-first
#pragma unroll
		for(int side = 0; side < 2; ++side)
		{
			const bool h = side ? h1 : h0;
			const int c = side ? c1 : c0;
			const int k = side ? k1 : k0;
			if(!h || c >= 0 || k == 0) continue;
			const int start = ~c;
			for(int q = start; q < start + k; ++q)
			{
				if(STATS) TRACE_STAT(++tests);
				const float4 *tp = C.tris + 3 * q;
				const float4 ta = tp[0], tb = tp[1], tc = tp[2];
				const float t = triTest(ta, tb, tc, o, d);
				if(t == -1.f) continue;
				const int prim = __float_as_int(tb.w);
				if(ANY && TS)
				{
					if(HIT_ANY_TS(t, prim, tmin, tmax, ts)) { t_best = t; prim_best = prim; return true; }
				}
				else if(ANY)
				{
					if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; return true; }
				}
				else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
				{
					t_best = t;
					prim_best = prim;
				}
			}
		}
		const bool i0 = h0 && c0 >= 0, i1 = h1 && c1 >= 0;
		if(i0 && i1)
		{
			const bool first0 = tn0 <= tn1;
			next = first0 ? c0 : c1;
			stackPush<kTraceBlock, false, false>(C, sp, lane, 0u, first0 ? c1 : c0);
			++sp;
		}
		else if(i0) next = c0;
		else if(i1) next = c1;
		if(next < 0)
		{
			if(sp == 0) break;
			--sp;
			next = stackPop<kTraceBlock, false, false>(C, sp, lane, 0u);
		}
		node = next;
	}
	return prim_best >= 0;
}

// ---------------------------------------------------------------------------------------------
// BVH4 (bvh.cc: collapsed binary SAH tree, 128 B nodes with the four child boxes in SoA form)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float lane4(const float4 &v, int k) { return k == 0 ? v.x : k == 1 ? v.y : k == 2 ? v.z : v.w; }

// The eight float4 of a node a visit reads: near / far planes per axis by the ray's selectors, the child
// links (>= 0: inner node, else ~first triangle slot) and the leaf triangle counts
struct Node4 { float4 nx, fx, ny, fy, nz, fz, cf, kf; };
__device__ __forceinline__ Node4 node4(const float4 *np, const SlabSel &sel)
{
	return Node4{np[sel.nx], np[sel.nx ^ 1], np[sel.ny], np[sel.ny ^ 1], np[sel.nz], np[sel.nz ^ 1], np[6], np[7]};
}
// float4 k at an LDS address through an explicit LDS pointer (the staged top treelets: ds_read, not flat loads)
__device__ __forceinline__ float4 ldsF4(const float4 *p, int k)
{
	typedef float V4 __attribute__((ext_vector_type(4)));
	typedef const __attribute__((address_space(3))) V4 *LdsV4;
	const V4 v = ((LdsV4)p)[k];
	return make_float4(v.x, v.y, v.z, v.w);
}

// Child k of the node against the ray (rayPrep's id, oid), culled to [box_t0, slack_t]: the entry and exit
// distances; the box is hit when lo <= hi
__device__ __forceinline__ void slab4(const Node4 &N, int k, V3 id, V3 oid, float box_t0, float slack_t, float &lo, float &hi)
{
	lo = fmaxf(fmaxf(__builtin_fmaf(lane4(N.nx, k), id.x, -oid.x), __builtin_fmaf(lane4(N.ny, k), id.y, -oid.y)),
	           fmaxf(__builtin_fmaf(lane4(N.nz, k), id.z, -oid.z), box_t0));
	hi = fminf(fminf(__builtin_fmaf(lane4(N.fx, k), id.x, -oid.x), __builtin_fmaf(lane4(N.fy, k), id.y, -oid.y)),
	           fminf(__builtin_fmaf(lane4(N.fz, k), id.z, -oid.z), slack_t));
}

__device__ __forceinline__ void cswap(float &ka, int &va, float &kb, int &vb)
{
	const bool sw = kb < ka;
	const float k = sw ? kb : ka;
	kb = sw ? ka : kb;
	ka = k;
	const int v = sw ? vb : va;
	vb = sw ? va : vb;
	va = v;
}

// Child order after a BVH4 visit (results never depend on it: closest hits tie-break on the primitive
// index, any hits answer occluded / not): closest rays sort the hit inner children by entry distance
// (5-exchange network; missed children and leaves have key inf), push the farther ones farthest first and
// descend the nearest; any-hit rays skip the network
__device__ __forceinline__ void sort4(float (&key)[4], int (&child)[4])
{
	cswap(key[0], child[0], key[1], child[1]);
	cswap(key[2], child[2], key[3], child[3]);
	cswap(key[0], child[0], key[2], child[2]);
	cswap(key[1], child[1], key[3], child[3]);
	cswap(key[1], child[1], key[2], child[2]);
}

// Same hit semantics as traverse2: leaf children are tested as soon as their box is hit, inner
// children are sorted by entry distance and descended nearest-first.  The lane's stack column is
// re-derived at every push / pop (stackPush's REMAT).
template<bool ANY, bool SPILL, bool TS = false, bool STATS = true>
__device__ bool traverse4(const TraceCtx &C, V3 o, V3 d, float tmin, float tmax, float &t_best, int &prim_best,
                          uint32_t &visits, uint32_t &tests, TsList *ts = nullptr)
{
	const RayPrep R = rayPrep(o, d, tmin, ANY);
	const float inf = __builtin_huge_valf();
	const uint32_t glane = blockIdx.x * blockDim.x + threadIdx.x;
	t_best = tmax;
	prim_best = -1;
	int sp = 0;
	int node = 0;
	// the first lds_depth levels live in LDS; deeper ones (rare) spill to this lane's HBM column
	auto push = [&](int v) { stackPush<kTraceBlock, SPILL, true>(C, sp, 0, glane, v); };
	// the box culling distance: recomputed only where t_best changes (a closest hit), not per visit
	float slack_t = slackOf(t_best);
	for(;;)
	{
		if(STATS) TRACE_STAT(++visits);
		const Node4 N = node4(C.nodes + 8 * node, R.sel);
		float key[4];
		int child[4], count[4];
		uint32_t leaves = 0;
		// the four slab tests first, so the node's registers are free before any triangle test
#pragma unroll
		for(int k = 0; k < 4; ++k)
		{
			float lo, hi;
			slab4(N, k, R.id, R.oid, R.box_t0, slack_t, lo, hi);
			// selects, not branches: a lane-varying `if` here costs an exec-mask save / restore per child
			const uint32_t h = lo <= hi ? 1u : 0u;
			child[k] = __float_as_int(lane4(N.cf, k));
			count[k] = __float_as_int(lane4(N.kf, k));
			const uint32_t inner = child[k] >= 0 ? 1u : 0u;
			key[k] = (h & inner) ? lo : inf;
			leaves |= (h & (inner ^ 1u) & (count[k] > 0 ? 1u : 0u)) << k;
		}
		// the hit leaves' triangles as one per-lane list (leaf order, then triangle order), so that a
		// wave runs max-over-lanes tests per node instead of one pass per leaf slot any lane hit
		int e[4], s4[4];
		{
			int acc = 0;
#pragma unroll
			for(int k = 0; k < 4; ++k)
			{
				const bool l = leaves & (1u << k);
				s4[k] = ~child[k] - acc;
				acc += l ? count[k] : 0;
				e[k] = acc;
			}
		}
		for(int i = 0; i < e[3]; ++i)
		{
			const int q = i + (i < e[0] ? s4[0] : i < e[1] ? s4[1] : i < e[2] ? s4[2] : s4[3]);
			{
				if(STATS) TRACE_STAT(++tests);
				const float4 *tp = C.tris + 3 * q;
				const float4 ta = tp[0], tb = tp[1], tc = tp[2];
				const float t = triTest(ta, tb, tc, o, d);
				if(t == -1.f) continue;
				const int prim = __float_as_int(tb.w);
				if(ANY && TS)
				{
					if(HIT_ANY_TS(t, prim, tmin, tmax, ts)) { t_best = t; prim_best = prim; return true; }
				}
				else if(ANY)
				{
					if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; return true; }
				}
				else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
				{
					t_best = t;
					prim_best = prim;
					slack_t = slackOf(t_best);
				}
			}
		}
		int next;
		if constexpr(ANY)
		{
			// any hit: the answer does not depend on the order the hit children are visited in (there is
			// no distance to cull against), so no sorting network — the first hit inner child is descended,
			// the others pushed in node order
			next = -1;
#pragma unroll
			for(int k = 0; k < 4; ++k)
			{
				if(!(key[k] < inf)) continue;
				if(next < 0) next = child[k];
				else { push(child[k]); ++sp; }
			}
		}
		else
		{
			sort4(key, child);
			if(key[3] < inf) { push(child[3]); ++sp; }
			if(key[2] < inf) { push(child[2]); ++sp; }
			if(key[1] < inf) { push(child[1]); ++sp; }
			next = key[0] < inf ? child[0] : -1;
		}
		if(next < 0)
		{
			if(sp == 0) break;
			--sp;
			next = stackPop<kTraceBlock, SPILL, true>(C, sp, 0, glane);
		}
		node = next;
	}
	return prim_best >= 0;
}

// traverse4 with the leaf triangle tests deferred (LDS-resident BVH4, no spill column, opaque shadows;
// DevQueues::trace_defer).  traverse4 tests a hit leaf's triangles inside the visit, so a wave pays the
// largest per-lane triangle count of every visit; here a visit only records its hit leaves in the lane's
// list (LDS, [slot][lane], one 16-bit entry per leaf: first triangle slot in the low kDeferStartBits bits,
// triangle count above), and the recorded triangles are tested afterwards in one dense loop per lane:
//   phase 1: visits as in traverse4 (slab tests, box_t0, slack_t, child order, stack) while the lane is
//            still traversing and its list has room for the four leaves a visit can add;
//   phase 2: the lane's pending triangles through triTest and traverse4's hit predicates; an any-hit ray
//            ends at its first hit, a closest hit tightens slack_t for the visits after a flush.
// A lane leaves phase 1 because its own traversal ended or its own list is full, never because of a
// neighbour, so a ray's visits and tests are a function of the ray and the capacity alone (the statistics
// do not depend on how the waves are composed).  Box culling sees t_best only after a flush — a ray visits
// a superset of traverse4's nodes — and the result is the same: closest hits are the minimum over
// (t, primitive) of the tested triangles, any hits a boolean.
constexpr int kDeferStartBits = 10;                      // scenes of < 1024 triangles (an LDS-resident scene holds <= 1024: 48 KB)
constexpr int kDeferMaxLeaf = (1 << (16 - kDeferStartBits)) - 1;
constexpr int kDeferRoom = 4;                            // free entries a visit needs (= the smallest capacity)
template<bool ANY, bool STATS>
__device__ bool traverse4Defer(const TraceCtx &C, uint16_t *list, int cap, V3 o, V3 d, float tmin, float tmax, float &t_best,
                               int &prim_best, uint32_t &visits, uint32_t &tests)
{
	const RayPrep R = rayPrep(o, d, tmin, ANY);
	const float inf = __builtin_huge_valf();
	t_best = tmax;
	prim_best = -1;
	int sp = 0;
	int node = 0;   // -1: the traversal has ended
	int n = 0;      // pending list entries
	auto push = [&](int v) { stackPush<kTraceBlock, false, true>(C, sp, 0, 0u, v); };
	float slack_t = slackOf(t_best);
	for(;;)
	{
		// ---- phase 1: box traversal, hit leaves recorded ----
		while(node >= 0 && n + kDeferRoom <= cap)
		{
			if(STATS) TRACE_STAT(++visits);
			const Node4 N = node4(C.nodes + 8 * node, R.sel);
			float key[4];
			int child[4];
			uint16_t *lp = list + n * kTraceBlock + stackColumn<true>(C, 0);
#pragma unroll
			for(int k = 0; k < 4; ++k)
			{
				float lo, hi;
				slab4(N, k, R.id, R.oid, R.box_t0, slack_t, lo, hi);
				const uint32_t h = lo <= hi ? 1u : 0u;
				child[k] = __float_as_int(lane4(N.cf, k));
				const int count = __float_as_int(lane4(N.kf, k));
				const uint32_t inner = child[k] >= 0 ? 1u : 0u;
				key[k] = (h & inner) ? lo : inf;
				// every child's entry is stored at the lane's next slot and kept only where the child is a hit
				// leaf (the slot then advances; n + 4 <= cap holds on entry): no lane-varying branch per child
				const uint32_t leaf = h & (inner ^ 1u) & (count > 0 ? 1u : 0u);
				*lp = (uint16_t)((uint32_t)~child[k] | ((uint32_t)count << kDeferStartBits));
				lp += leaf ? kTraceBlock : 0;
				n += (int)leaf;
			}
			int next;
			if constexpr(ANY)
			{
				next = -1;
#pragma unroll
				for(int k = 0; k < 4; ++k)
				{
					if(!(key[k] < inf)) continue;
					if(next < 0) next = child[k];
					else { push(child[k]); ++sp; }
				}
			}
			else
			{
				sort4(key, child);
				if(key[3] < inf) { push(child[3]); ++sp; }
				if(key[2] < inf) { push(child[2]); ++sp; }
				if(key[1] < inf) { push(child[1]); ++sp; }
				next = key[0] < inf ? child[0] : -1;
			}
			if(next < 0 && sp > 0)
			{
				--sp;
				next = stackPop<kTraceBlock, false, true>(C, sp, 0, 0u);
			}
			node = next;
		}
		// ---- phase 2: the pending leaves' triangles, one per trip whatever leaf they belong to ----
		// (last recorded leaf first: n is the loop's only index, and no result depends on the order)
		uint32_t ent = 0;   // the leaf being tested: next triangle slot | triangles left << kDeferStartBits
		for(;;)
		{
			if((ent >> kDeferStartBits) == 0)
			{
				if(n == 0) break;
				--n;
				ent = list[n * kTraceBlock + stackColumn<true>(C, 0)];
			}
			if(STATS) TRACE_STAT(++tests);
			const float4 *tp = C.tris + 3 * (ent & ((1u << kDeferStartBits) - 1u));
			const float4 ta = tp[0], tb = tp[1], tc = tp[2];
			ent += 1u - (1u << kDeferStartBits);   // (the slot of a leaf's last triangle + 1 <= 1023: no carry into the count)
			const float t = triTest(ta, tb, tc, o, d);
			if(t == -1.f) continue;
			const int prim = __float_as_int(tb.w);
			if(ANY)
			{
				if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; node = -1; break; }
			}
			else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
			{
				t_best = t;
				prim_best = prim;
				slack_t = slackOf(t_best);
			}
		}
		n = 0;
		if(node < 0) break;
	}
	return prim_best >= 0;
}

// The flat scan (LDS-resident BVH4 over at most kFlatMaxTris triangles, no spill column, opaque shadows;
// DevQueues::trace_flat): no box traversal at all.
//   phase 1: every leaf box of the scene (bvh.h FlatLeaf, built by upload()) against the ray's
//            [box_t0, slackOf(tmax)] interval, in a loop that is the same for every lane: no stack, no child
//            order, no per-lane address.  The record index is wave-uniform and the table is read through the
//            constant address space, so a record arrives as one scalar load for the 64 lanes, two records
//            requested per trip.  Per axis t_a = fma(lo, id, -oid),
//            t_b = fma(hi, id, -oid), near = min, far = max: by the monotonicity argument above slab4 these
//            are the values slab4's sign-selected planes give, so a box is hit here exactly when slab4 hits it
//            with slack_t = slackOf(tmax).  A hit box ORs the leaf's triangle slots into the lane's 64-bit
//            mask; the table is ordered so that each of the three loops knows which mask words it touches.
//   phase 2: the mask's triangles, lowest slot first, through triTest and traverse4's hit predicates; an
//            any-hit ray ends at its first hit.  One round per ray: t_best never culls a box.
// A leaf's stored box lies inside its ancestors' stored boxes (every box is its subtree's bounds plus a pad
// that grows with the bounds, bvh.cc padBox), so the hit leaves are a superset of the leaves either tree loop reaches with the same interval;
// closest hits are the minimum over (t, primitive) of the tested triangles, any hits a boolean: the results
// are traverse4's.  A ray's tests depend on the ray and the scene alone.  STATS: a "visit" is four boxes.
typedef float f32x8_t __attribute__((ext_vector_type(8)));
__device__ __forceinline__ f32x8_t flatLd(const float4 *__restrict__ tab, int i)
{
#ifdef __HIP_DEVICE_COMPILE__
	typedef const f32x8_t __attribute__((address_space(4))) *ConstRec;
	return ((ConstRec)tab)[__builtin_amdgcn_readfirstlane(i)];
#else   // (host pass of the single-source compile: never executed)
	return reinterpret_cast<const f32x8_t *>(tab)[i];
#endif
}
// one record against the ray: WORDS bit 0 = the leaf has slots in the low mask word, bit 1 = in the high one
template<int WORDS>
__device__ __forceinline__ void flatBox(const f32x8_t &r, const RayPrep &R, float t_far, uint32_t &m_lo, uint32_t &m_hi)
{
	const float ax = __builtin_fmaf(r[0], R.id.x, -R.oid.x), bx = __builtin_fmaf(r[4], R.id.x, -R.oid.x);
	const float ay = __builtin_fmaf(r[1], R.id.y, -R.oid.y), by = __builtin_fmaf(r[5], R.id.y, -R.oid.y);
	const float az = __builtin_fmaf(r[2], R.id.z, -R.oid.z), bz = __builtin_fmaf(r[6], R.id.z, -R.oid.z);
	const float lo = fmaxf(fmaxf(fmaxf(fminf(ax, bx), fminf(ay, by)), fminf(az, bz)), R.box_t0);
	const float hi = fminf(fminf(fminf(fmaxf(ax, bx), fmaxf(ay, by)), fmaxf(az, bz)), t_far);
	const bool h = lo <= hi;
	if(WORDS & 1) m_lo |= h ? __float_as_uint(r[3]) : 0u;
	if(WORDS & 2) m_hi |= h ? __float_as_uint(r[7]) : 0u;
}
// records [i0, i1), two per trip: both records are requested before the first is tested
template<int WORDS>
__device__ __forceinline__ void flatScan(const float4 *__restrict__ tab, int i0, int i1, const RayPrep &R, float t_far, uint32_t &m_lo,
                                         uint32_t &m_hi)
{
	int i = i0;
	for(; i + 1 < i1; i += 2)
	{
		const f32x8_t r0 = flatLd(tab, i), r1 = flatLd(tab, i + 1);
		flatBox<WORDS>(r0, R, t_far, m_lo, m_hi);
		flatBox<WORDS>(r1, R, t_far, m_lo, m_hi);
	}
	if(i < i1) flatBox<WORDS>(flatLd(tab, i), R, t_far, m_lo, m_hi);
}
template<bool ANY, bool STATS>
__device__ bool traverseFlat(const TraceCtx &C, const float4 *__restrict__ tab, int flat, V3 o, V3 d, float tmin, float tmax, float &t_best,
                             int &prim_best, uint32_t &visits, uint32_t &tests)
{
	const RayPrep R = rayPrep(o, d, tmin, ANY);
	t_best = tmax;
	prim_best = -1;
	// ---- phase 1: the leaf boxes (flat = bvh.h flatPack: n | n_lo << 8 | n_mid << 16) ----
	const int n = flat & 0xff, n_lo = (flat >> 8) & 0xff, n_mid = (flat >> 16) & 0xff;
	const float t_far = slackOf(tmax);
	uint32_t m_lo = 0, m_hi = 0;
	flatScan<1>(tab, 0, n_lo, R, t_far, m_lo, m_hi);
	flatScan<3>(tab, n_lo, n_mid, R, t_far, m_lo, m_hi);
	flatScan<2>(tab, n_mid, n, R, t_far, m_lo, m_hi);
	if(STATS) TRACE_STAT(visits += (uint32_t)(n + 3) >> 2);
	// ---- phase 2: the pending triangles, one per trip; the bit index is the triangle slot ----
	uint64_t m = ((uint64_t)m_hi << 32) | m_lo;
	while(m)
	{
		const int q = __builtin_ctzll(m);
		m &= m - 1ull;
		if(STATS) TRACE_STAT(++tests);
		const float4 *tp = C.tris + 3 * q;
		const float4 ta = tp[0], tb = tp[1], tc = tp[2];
		const float t = triTest(ta, tb, tc, o, d);
		if(t == -1.f) continue;
		const int prim = __float_as_int(tb.w);
		if(ANY)
		{
			if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; break; }
		}
		else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
		{
			t_best = t;
			prim_best = prim;
		}
	}
	return prim_best >= 0;
}

// k_trace's BVH4 loop with per-lane ray refill: a lane works through its own sequence of queue
// entries (j, j + stride, ...), closest rays then shadow rays, and starts its next ray as soon as
// its traversal ends, so a wave runs as long as its longest lane's sum of rays instead of the sum
// over rays of the longest lane.  Every ray runs the sequence of traverse4 (same visits, culling,
// leaf order and early exits), so hits are identical.  The slack is recomputed per visit, a hit leaf
// without triangles adds a zero count to the span, the stack column is threadIdx.x.
template<bool SPILL, bool STATS = true>
__device__ void traceRefill4(const TraceCtx &C, const DevQueues &Q, const DevPaths &P, uint32_t n_a, uint32_t total,
                             uint32_t a0, uint32_t s0, uint32_t j, uint32_t stride, uint32_t &visits, uint32_t &tests,
                             uint32_t &n_closest, uint32_t &n_shadow)
{
	const int lane = threadIdx.x;
	const uint32_t glane = blockIdx.x * blockDim.x + threadIdx.x;
	const float inf = __builtin_huge_valf();
	V3 o = v3(0.f, 0.f, 0.f), d = o, id = o, oid = o;
	SlabSel sel{0, 2, 4};
	float tmin = 0.f, tmax = 0.f, box_t0 = 0.f, t_best = 0.f;
	int prim_best = -1, sp = 0, node = -1;
	bool any = false;
	uint32_t cur = 0;
	auto push = [&](int v) { stackPush<kTraceBlock, SPILL, false>(C, sp, lane, glane, v); };
	for(;;)
	{
		if(node < 0)
		{
			// next ray of this lane (closest entries with a NaN direction carry no ray)
			bool got = false;
			for(;;)
			{
				if(j >= total) break;
				cur = j;
				j += stride;
				if(cur < n_a)
				{
					float tw;
					if(!loadQRay(Q, a0 + cur, o, d, tmin, tw)) continue;
					tmax = (tw >= 0.f) ? tw : inf;
					any = false;
					++n_closest;
				}
				else
				{
					const float4 od = rayLd4(&Q.sh_o[s0 + (cur - n_a)]);
					const float4 dd = rayLd4(&Q.sh_d[s0 + (cur - n_a)]);
					o = xyz(od);
					d = xyz(dd);
					tmin = 0.f;
					tmax = dd.w;
					any = true;
					++n_shadow;
				}
				got = true;
				break;
			}
			if(!got) break;
			const RayPrep R = rayPrep(o, d, tmin, any);
			id = R.id;
			oid = R.oid;
			sel = R.sel;
			box_t0 = R.box_t0;
			t_best = tmax;
			prim_best = -1;
			sp = 0;
			node = 0;
		}
		if(STATS) TRACE_STAT(++visits);
		// (the top treelet from LDS; the members are loaded in place: selecting between two node4() results
		// changed the order of this loop's mask operations)
		Node4 N;
		if(node < C.n_top)
		{
			const float4 *tp = C.top + kTopStride * node;
			N.nx = ldsF4(tp, sel.nx); N.fx = ldsF4(tp, sel.nx ^ 1); N.ny = ldsF4(tp, sel.ny); N.fy = ldsF4(tp, sel.ny ^ 1); N.nz = ldsF4(tp, sel.nz); N.fz = ldsF4(tp, sel.nz ^ 1); N.cf = ldsF4(tp, 6); N.kf = ldsF4(tp, 7);
		}
		else
		{
			const float4 *np = C.nodes + 8 * node;
			N.nx = np[sel.nx]; N.fx = np[sel.nx ^ 1]; N.ny = np[sel.ny]; N.fy = np[sel.ny ^ 1]; N.nz = np[sel.nz]; N.fz = np[sel.nz ^ 1]; N.cf = np[6]; N.kf = np[7];
		}
		const float slack_t = slackOf(t_best);
		float key[4];
		int child[4], e[4], s4[4];
		int acc = 0;
#pragma unroll
		for(int k = 0; k < 4; ++k)
		{
			float lo, hi;
			slab4(N, k, id, oid, box_t0, slack_t, lo, hi);
			const uint32_t h = lo <= hi ? 1u : 0u;
			child[k] = __float_as_int(lane4(N.cf, k));
			const int count = __float_as_int(lane4(N.kf, k));
			const uint32_t inner = child[k] >= 0 ? 1u : 0u;
			key[k] = (h & inner) ? lo : inf;
			s4[k] = ~child[k] - acc;
			acc += (h & (inner ^ 1u)) ? count : 0;
			e[k] = acc;
		}
		bool done = false;
		for(int i = 0; i < e[3]; ++i)
		{
			const int q = i + (i < e[0] ? s4[0] : i < e[1] ? s4[1] : i < e[2] ? s4[2] : s4[3]);
			if(STATS) TRACE_STAT(++tests);
			const float4 *tp = C.tris + 3 * q;
			const float4 ta = tp[0], tb = tp[1], tc = tp[2];
			const float t = triTest(ta, tb, tc, o, d);
			if(t == -1.f) continue;
			const int prim = __float_as_int(tb.w);
			if(any)
			{
				if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; done = true; break; }
			}
			else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
			{
				t_best = t;
				prim_best = prim;
			}
		}
		if(!done)
		{
			sort4(key, child);
			if(key[3] < inf) { push(child[3]); ++sp; }
			if(key[2] < inf) { push(child[2]); ++sp; }
			if(key[1] < inf) { push(child[1]); ++sp; }
			int next = key[0] < inf ? child[0] : -1;
			if(next < 0 && sp > 0)
			{
				--sp;
				next = stackPop<kTraceBlock, SPILL, false>(C, sp, lane, glane);
			}
			node = next;
			done = next < 0;
		}
		if(done)
		{
			// (the NEE entry of an opaque shadow ray rides in sh_o.w: re-read at the end rather than held
			// in a register through the traversal, which spilled at this kernel's 6-wave budget)
			if(any) P.occ[__float_as_int(Q.sh_o[s0 + (cur - n_a)].w)] = prim_best >= 0 ? 1 : 0;   // P = state set of the consumer shade
			else
			{
				raySt(&Q.hit_t[a0 + cur], t_best);
				raySt(&Q.hit_prim[a0 + cur], prim_best);
			}
			node = -1;
		}
	}
}

// ---- quantised BVH8 (bvhgpu.hip k_q8_write: the device-built tree collapsed to eight children, child
// boxes as bytes over a per-node origin and power-of-two quanta, rounded outwards; opt-in for scenes in
// global memory).  A visit reads 80 B (one line): origin, quanta, child masks, the first inner child, the
// first leaf triangle (the BVH8's own triangle array, leaves in node order) and the six byte planes;
// the slab test decodes t = q · (2^e / d) + (origin − o) / d.  The decoded boxes contain the float boxes
// (which carry the BVH4's padding), the triangle test and the tie rule are the BVH4's: the same hits.
constexpr int kTop8Stride = 5;   // float4 per staged node in LDS (the 80 B a visit reads: 20 dwords, so 16
                                 // consecutive nodes start on 16 distinct bank quads)
__device__ __forceinline__ float q8Byte(uint32_t lo4, uint32_t hi4, int k)
{
	const uint32_t w = k < 4 ? lo4 : hi4;
	return (float)((w >> (8 * (k & 3))) & 0xffu);   // (v_cvt_f32_ubyteN)
}

// Batcher's odd-even merge network (19 compare-exchanges) over the eight children's entry keys
__device__ __forceinline__ void sort8(float (&key)[8], int (&child)[8])
{
	cswap(key[0], child[0], key[1], child[1]); cswap(key[2], child[2], key[3], child[3]);
	cswap(key[4], child[4], key[5], child[5]); cswap(key[6], child[6], key[7], child[7]);
	cswap(key[0], child[0], key[2], child[2]); cswap(key[1], child[1], key[3], child[3]);
	cswap(key[4], child[4], key[6], child[6]); cswap(key[5], child[5], key[7], child[7]);
	cswap(key[1], child[1], key[2], child[2]); cswap(key[5], child[5], key[6], child[6]);
	cswap(key[0], child[0], key[4], child[4]); cswap(key[1], child[1], key[5], child[5]);
	cswap(key[2], child[2], key[6], child[6]); cswap(key[3], child[3], key[7], child[7]);
	cswap(key[2], child[2], key[4], child[4]); cswap(key[3], child[3], key[5], child[5]);
	cswap(key[1], child[1], key[2], child[2]); cswap(key[3], child[3], key[4], child[4]);
	cswap(key[5], child[5], key[6], child[6]);
}

// The refill loop over the BVH8 (closest entries through Q.perm when rays are binned).  The slack is
// recomputed per visit, the stack column is re-derived.
template<bool SPILL, bool STATS = true>
__device__ void traceRefill8(const TraceCtx &C, const DevQueues &Q, const DevPaths &P, uint32_t n_a, uint32_t total,
                             uint32_t a0, uint32_t s0, uint32_t j, uint32_t stride, uint32_t &visits, uint32_t &tests,
                             uint32_t &n_closest, uint32_t &n_shadow)
{
	const uint32_t glane = blockIdx.x * blockDim.x + threadIdx.x;
	const float inf = __builtin_huge_valf();
	V3 o = v3(0.f, 0.f, 0.f), d = o, id = o;
	float tmin = 0.f, tmax = 0.f, box_t0 = 0.f, t_best = 0.f;
	int prim_best = -1, sp = 0, node = -1;
	bool any = false;
	uint32_t cur = 0;
	auto push = [&](int v) { stackPush<kTraceBlock, SPILL, true>(C, sp, 0, glane, v); };
	for(;;)
	{
		if(node < 0)
		{
			bool got = false;
			for(;;)
			{
				if(j >= total) break;
				cur = j;
				j += stride;
				if(cur < n_a)
				{
					float tw;
					// (ray binning: the entry's ray and hit live at the permuted queue address)
					if(Q.perm) cur = Q.perm[a0 + cur] - a0;
					if(!loadQRay(Q, a0 + cur, o, d, tmin, tw)) continue;
					tmax = (tw >= 0.f) ? tw : inf;
					any = false;
					++n_closest;
				}
				else
				{
					const float4 od = rayLd4(&Q.sh_o[s0 + (cur - n_a)]);
					const float4 dd = rayLd4(&Q.sh_d[s0 + (cur - n_a)]);
					o = xyz(od);
					d = xyz(dd);
					tmin = 0.f;
					tmax = dd.w;
					any = true;
					++n_shadow;
				}
				got = true;
				break;
			}
			if(!got) break;
			const RayPrep R = rayPrep(o, d, tmin, any);
			id = R.id;
			box_t0 = R.box_t0;
			t_best = tmax;
			prim_best = -1;
			sp = 0;
			node = 0;
		}
		if(STATS) TRACE_STAT(++visits);
		float4 n0, n1, n2, n3, n4;
		if(node < C.n_top)
		{
			const float4 *tp = C.top + kTop8Stride * node;
			n0 = ldsF4(tp, 0); n1 = ldsF4(tp, 1); n2 = ldsF4(tp, 2); n3 = ldsF4(tp, 3); n4 = ldsF4(tp, 4);
		}
		else
		{
			const float4 *np = C.nodes + 8 * node;
			n0 = np[0]; n1 = np[1]; n2 = np[2]; n3 = np[3]; n4 = np[4];
		}
		const uint32_t meta = __float_as_uint(n0.w);
		const uint32_t inner = meta >> 24, leaf = __float_as_uint(n1.x) & 0xffu;
		const int inner_base = __float_as_int(n1.y), tri_base = __float_as_int(n1.z);
		// per axis: t of plane q = q * A + B (A = 2^e / d, B = (origin - o) / d), near / far byte rows by the sign of 1/d
		const float ax = __uint_as_float((meta & 0xffu) << 23) * id.x, ay = __uint_as_float(((meta >> 8) & 0xffu) << 23) * id.y,
		            az = __uint_as_float(((meta >> 16) & 0xffu) << 23) * id.z;
		const float bx = (n0.x - o.x) * id.x, by = (n0.y - o.y) * id.y, bz = (n0.z - o.z) * id.z;
		const bool px = id.x >= 0.f, py = id.y >= 0.f, pz = id.z >= 0.f;
		const uint32_t nx0 = __float_as_uint(px ? n2.x : n2.z), nx1 = __float_as_uint(px ? n2.y : n2.w);
		const uint32_t fx0 = __float_as_uint(px ? n2.z : n2.x), fx1 = __float_as_uint(px ? n2.w : n2.y);
		const uint32_t ny0 = __float_as_uint(py ? n3.x : n3.z), ny1 = __float_as_uint(py ? n3.y : n3.w);
		const uint32_t fy0 = __float_as_uint(py ? n3.z : n3.x), fy1 = __float_as_uint(py ? n3.w : n3.y);
		const uint32_t nz0 = __float_as_uint(pz ? n4.x : n4.z), nz1 = __float_as_uint(pz ? n4.y : n4.w);
		const uint32_t fz0 = __float_as_uint(pz ? n4.z : n4.x), fz1 = __float_as_uint(pz ? n4.w : n4.y);
		const float slack_t = slackOf(t_best);
		float key[8];
		int child[8];
		uint32_t leaves = 0;
#pragma unroll
		for(int k = 0; k < 8; ++k)
		{
			const float lo = fmaxf(fmaxf(__builtin_fmaf(q8Byte(nx0, nx1, k), ax, bx), __builtin_fmaf(q8Byte(ny0, ny1, k), ay, by)),
			                       fmaxf(__builtin_fmaf(q8Byte(nz0, nz1, k), az, bz), box_t0));
			const float hi = fminf(fminf(__builtin_fmaf(q8Byte(fx0, fx1, k), ax, bx), __builtin_fmaf(q8Byte(fy0, fy1, k), ay, by)),
			                       fminf(__builtin_fmaf(q8Byte(fz0, fz1, k), az, bz), slack_t));
			const uint32_t h = lo <= hi ? 1u : 0u;
			const uint32_t isi = (inner >> k) & 1u;
			key[k] = (h & isi) ? lo : inf;
			child[k] = inner_base + __builtin_popcount(inner & ((1u << k) - 1u));
			leaves |= (h & (leaf >> k) & 1u) << k;
		}
		bool done = false;
		for(uint32_t m = leaves; m; m &= m - 1u)
		{
			const int k = __builtin_ctz(m);
			const int q = tri_base + __builtin_popcount(leaf & ((1u << k) - 1u));
			if(STATS) TRACE_STAT(++tests);
			const float4 *tp = C.tris + 3 * q;
			const float4 ta = tp[0], tb = tp[1], tc = tp[2];
			const float t = triTest(ta, tb, tc, o, d);
			if(t == -1.f) continue;
			const int prim = __float_as_int(tb.w);
			if(any)
			{
				if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; done = true; break; }
			}
			else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
			{
				t_best = t;
				prim_best = prim;
			}
		}
		if(!done)
		{
			// nearest child descended first, the others pushed farthest first
			sort8(key, child);
#pragma unroll
			for(int k = 7; k >= 1; --k)
				if(key[k] < inf) { push(child[k]); ++sp; }
			int next = key[0] < inf ? child[0] : -1;
			if(next < 0 && sp > 0)
			{
				--sp;
				next = stackPop<kTraceBlock, SPILL, true>(C, sp, 0, glane);
			}
			node = next;
			done = next < 0;
		}
		if(done)
		{
			if(any) P.occ[__float_as_int(Q.sh_o[s0 + (cur - n_a)].w)] = prim_best >= 0 ? 1 : 0;
			else
			{
				raySt(&Q.hit_t[a0 + cur], t_best);
				raySt(&Q.hit_prim[a0 + cur], prim_best);
			}
			node = -1;
		}
	}
}

template<bool ANY, bool WIDE, bool SPILL = true, bool TS = false, bool STATS = true>
__device__ __forceinline__ bool traverse(const TraceCtx &C, V3 o, V3 d, float tmin, float tmax, float &t_best,
                                         int &prim_best, uint32_t &visits, uint32_t &tests, TsList *ts = nullptr)
{
	if(WIDE) return traverse4<ANY, SPILL, TS, STATS>(C, o, d, tmin, tmax, t_best, prim_best, visits, tests, ts);
	return traverse2<ANY, TS, STATS>(C, o, d, tmin, tmax, t_best, prim_best, visits, tests, ts);
}

// The rays one k_path lane owes before its next vertex: the shadow rays its last NEE recorded
// (rec entries with `want`, when `shadows`) and its closest ray (when `closest`).  traceRefill4's
// scheme: one BVH4 visit per loop trip and a lane starts its next ray as soon as one ends, so the
// wave runs for its busiest lane's sum of traversals (not one full traversal per ray slot, most of
// whose lanes would idle: the MIS material-sample shadow ray exists for a few lanes only).  Every ray
// runs traverse4's exact sequence of visits, culling, leaf order and exits: hits are identical.
// The stack has LDS levels only, STRIDE lanes per level, at column threadIdx.x.
template<bool STATS, int STRIDE = kTraceBlock>
__device__ __forceinline__ void traceLaneRays(const TraceCtx &C, const float4 *rec, uint8_t *occ, int K, bool shadows, bool closest, V3 co,
                                              V3 cd, float ctmin, float ctmax, float &hit_t, int &hit_prim, uint32_t &visits,
                                              uint32_t &tests, uint32_t &n_closest, uint32_t &n_shadow)
{
	const int lane = threadIdx.x;
	const float inf = __builtin_huge_valf();
	V3 o = v3(0.f, 0.f, 0.f), d = o, id = o, oid = o;
	SlabSel sel{0, 2, 4};
	float tmax = 0.f, tmin = 0.f, box_t0 = 0.f, t_best = 0.f;
	int prim_best = -1, sp = 0, node = -1, cur = 0;
	int e = shadows ? 0 : K;
	bool any = false, cl = closest;
	for(;;)
	{
		if(node < 0)
		{
			// this lane's next ray: the recorded shadow rays in entry order, then the closest ray
			bool got = false;
			while(e < K)
			{
				const int ee = e++;
				const float4 dd = rec[2 * ee + 1];
				if(dd.w == 0.f) continue;
				const float4 od = rec[2 * ee];
				o = xyz(od);
				d = xyz(dd);
				tmin = 0.f;
				tmax = od.w;
				any = true;
				cur = ee;
				++n_shadow;
				got = true;
				break;
			}
			if(!got && cl)
			{
				cl = false;
				o = co;
				d = cd;
				tmin = ctmin;
				tmax = ctmax;
				any = false;
				++n_closest;
				got = true;
			}
			if(!got) break;
			const RayPrep R = rayPrep(o, d, tmin, any);
			id = R.id;
			oid = R.oid;
			sel = R.sel;
			box_t0 = R.box_t0;
			t_best = tmax;
			prim_best = -1;
			sp = 0;
			node = 0;
		}
		if(STATS) TRACE_STAT(++visits);
		const Node4 N = node4(C.nodes + 8 * node, sel);
		const float slack_t = slackOf(t_best);
		float key[4];
		int child[4], e4[4], s4[4];
		int acc = 0;
#pragma unroll
		for(int k = 0; k < 4; ++k)
		{
			float lo, hi;
			slab4(N, k, id, oid, box_t0, slack_t, lo, hi);
			const uint32_t h = lo <= hi ? 1u : 0u;
			child[k] = __float_as_int(lane4(N.cf, k));
			const int count = __float_as_int(lane4(N.kf, k));
			const uint32_t inner = child[k] >= 0 ? 1u : 0u;
			key[k] = (h & inner) ? lo : inf;
			s4[k] = ~child[k] - acc;
			acc += (h & (inner ^ 1u)) ? count : 0;
			e4[k] = acc;
		}
		bool done = false;
		for(int i = 0; i < e4[3]; ++i)
		{
			const int q = i + (i < e4[0] ? s4[0] : i < e4[1] ? s4[1] : i < e4[2] ? s4[2] : s4[3]);
			if(STATS) TRACE_STAT(++tests);
			const float4 *tp = C.tris + 3 * q;
			const float4 ta = tp[0], tb = tp[1], tc = tp[2];
			const float t = triTest(ta, tb, tc, o, d);
			if(t == -1.f) continue;
			const int prim = __float_as_int(tb.w);
			if(any)
			{
				if(HIT_ANY(t, tmax)) { t_best = t; prim_best = prim; done = true; break; }
			}
			else if(HIT_CLOSER(t, prim, tmin, t_best, prim_best))
			{
				t_best = t;
				prim_best = prim;
			}
		}
		if(!done)
		{
			sort4(key, child);
			if(key[3] < inf) { stackPush<STRIDE, false, false>(C, sp, lane, 0u, child[3]); ++sp; }
			if(key[2] < inf) { stackPush<STRIDE, false, false>(C, sp, lane, 0u, child[2]); ++sp; }
			if(key[1] < inf) { stackPush<STRIDE, false, false>(C, sp, lane, 0u, child[1]); ++sp; }
			int next = key[0] < inf ? child[0] : -1;
			if(next < 0 && sp > 0)
			{
				--sp;
				next = stackPop<STRIDE, false, false>(C, sp, lane, 0u);
			}
			node = next;
			done = next < 0;
		}
		if(done)
		{
			if(any) occ[cur] = prim_best >= 0 ? 1 : 0;
			else
			{
				hit_t = t_best;
				hit_prim = prim_best;
			}
			node = -1;
		}
	}
}

// Every triangle of a scene of at most kBruteTris tested in order (k_trace_brute): the reference's own
// AcceleratorSimpleTest semantics, which equal the BVH's by construction.  The triangle loop is wave-uniform:
// the vertices come through scalar loads shared by the 64 lanes.
#ifdef YAF_EXPERIMENTS
template<bool ANY>
__device__ __forceinline__ bool bruteTrace(const float4 *__restrict__ tris, int n_tris, V3 o, V3 d, float tmin, float tmax, float &t_best,
                                           int &prim_best, uint32_t &tests, bool active)
{
	t_best = tmax;
	prim_best = -1;
	bool hit = false;
	for(int q = 0; q < n_tris; ++q)
	{
		// wave-uniform index through the constant address space -> scalar loads (the K$ holds the
		// whole scene)
#ifdef __HIP_DEVICE_COMPILE__
		typedef const float4 __attribute__((address_space(4))) *ConstF4;
		const ConstF4 ct = (ConstF4)tris;
		const int qs = __builtin_amdgcn_readfirstlane(q);
		const float4 ta = ct[3 * qs], tb = ct[3 * qs + 1], tc = ct[3 * qs + 2];
#else   // (host pass of the single-source compile: never executed)
		const float4 ta = tris[3 * q], tb = tris[3 * q + 1], tc = tris[3 * q + 2];
#endif
		const float t = triTest(ta, tb, tc, o, d);
		const int prim = __float_as_int(tb.w);
		if(ANY)
		{
			if(!hit && t != -1.f && HIT_ANY(t, tmax)) { hit = true; t_best = t; prim_best = prim; }
			if((q & 3) == 3 && __all(hit || !active)) break;
		}
		else if(t != -1.f && HIT_CLOSER(t, prim, tmin, t_best, prim_best))
		{
			t_best = t;
			prim_best = prim;
		}
	}
	if(active) tests += (uint32_t)n_tris;
	return prim_best >= 0;
}
#endif   // YAF_EXPERIMENTS

}   // namespace yafamd
