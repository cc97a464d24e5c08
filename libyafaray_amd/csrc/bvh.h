// Host-side BVH builder for the GPU traversal kernels.
//
// Replaces the reference's accelerator build (AcceleratorKdTree::buildTree,
// src/accelerator/accelerator_kdtree.cc:420-628, SAH kd-tree with clipping).  The closest /
// any hit a traversal returns does not depend on the acceleration structure, so
// a binned-SAH BVH2 whose inner nodes store both child boxes (one 64 B fetch per step, two slab
// tests) is a legal drop-in that maps far better onto wave64 SIMD than pointer-chasing kd nodes.
#pragma once

#include <cstdint>
#include <vector>

namespace yafamd
{

struct BvhInput
{
	const float *verts;     // xyz per vertex
	const int *tris;        // 3 vertex indices per triangle
	int n_tris;
	float node_cost = 0.f;   // SAH node cost (<= 0: default 0.5)
	int width = 4;           // 2: BVH2 (4 float4 per node), 4: BVH4 (8 float4 per node)
};

// The device build's optional 8-wide collapse of the same binary tree, quantised (bvhgpu.hip k_q8_write:
// 8 float4 per node) with its own copy of the triangle records in node order; k_trace's refill loop
// traverses it for scenes in global memory (opt-in YAFARAY_AMD_BVH8=1).
struct YafBvh8
{
	void *nodes = nullptr;   // device memory, owned by the caller
	void *tris = nullptr;    // device memory (3 float4 per triangle), owned by the caller
	int n_nodes = 0, depth = 0, stack_need = 0;
};

struct BvhOutput
{
	std::vector<float> nodes;   // 16 (BVH2) or 32 (BVH4) floats per node (devscene.h layout)
	int width = 2;
	std::vector<float> tris;    // 12 floats per triangle, leaf order (devscene.h layout)
	int n_nodes = 0;
	int depth = 0;              // inner-node depth (bounds the traversal stack)
	int max_leaf = 0;
	int stack_need = 0;         // worst-case traversal stack entries (BVH4: sum of deferred siblings along a path)
};

// Builds the tree.  `threads` > 1 builds independent subtrees concurrently.
BvhOutput buildBvh(const BvhInput &in, int leaf_size = 4, int threads = 1);

// The leaf table of a BVH4 over at most kFlatMaxTris triangles (k_trace's flat scan, trace.h traverseFlat): one
// record per child slot that is a leaf with triangles, the child's box bit for bit as its parent node stores it
// and the leaf's triangle slots [first, first + count) as bits of a 64-bit word.
struct FlatLeaf
{
	float lo[3];
	uint32_t bits_lo;   // triangle slots 0 .. 31
	float hi[3];
	uint32_t bits_hi;   // triangle slots 32 .. 63
};
constexpr int kFlatMaxTris = 64;
// The automatic limit on the leaf count L: the L at which the scan's 19 VALU per leaf box (20 in the compiled
// loop) reach what the deferred leaf lists spend on their box traversal per wave on the wave model's Cornell mix
// (tools/trace_wave_sim.cc, last line: 753 VALU = 19 x 39.6).  Not measured beyond the Cornell box (21 leaves);
// YAFARAY_AMD_TRACE_FLAT=1 forces the scan whatever L.
constexpr int kFlatMaxLeaves = 39;
struct FlatTable
{
	// records ordered by first triangle slot: [0, n_lo) have bits in the low word only, [n_lo, n_mid) in both
	// (at most one leaf straddles slot 31 / 32), [n_mid, n) in the high word only; one zero record follows
	// the last (so an empty table is still an allocation)
	std::vector<FlatLeaf> rec;
	int n = 0, n_lo = 0, n_mid = 0;
};
// The table of the BVH4 `nodes` (32 floats per node); empty (n == 0) when a leaf reaches past slot 63.
FlatTable buildFlatTable(const float *nodes, int n_nodes);
// Whether k_trace may run the flat scan on a tree of n_tris triangles in n_leaves leaves (forced: whatever L)
bool flatEligible(int n_tris, int n_leaves, bool forced);
// n | n_lo << 8 | n_mid << 16: DevQueues::trace_flat
inline int flatPack(const FlatTable &t) { return t.n | (t.n_lo << 8) | (t.n_mid << 16); }

// The triangle record exactly as the device test consumes it (primitive_triangle.cc:47-49):
// v0, e1 = v1 - v0, e2 = v2 - v0, eps = 0.1f * min_raydist * max(|e1|, |e2|).
void packTriangle(const float *v0, const float *v1, const float *v2, int prim, float *out12);

} // namespace yafamd
