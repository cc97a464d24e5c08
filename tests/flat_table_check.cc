// Host check of the leaf table of k_trace's flat scan (libyafaray_amd/csrc/bvh.cc buildFlatTable) on the
// project's own BVH4 (buildBvh with the leaf size given) over a mesh read from a file: the table holds every
// triangle slot exactly once, every record's box equals its parent's stored child box bit for bit, the leaf count
// and the three word ranges are as the tree says, one zero record follows the last, and the eligibility
// function refuses 65 triangles and a leaf count above the limit.
//   flat_table_check MESH LEAF_SIZE      MESH: int32 n_verts, int32 n_tris, float32 verts[3 n_verts], int32 tris[3 n_tris]
// Build: g++ -O2 -std=c++17 flat_table_check.cc ../libyafaray_amd/csrc/bvh.cc -lpthread
#include "../libyafaray_amd/csrc/bvh.h"

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace yafamd;

static int fails = 0;
#define CHECK(c, ...) do { if(!(c)) { ++fails; if(fails < 20) { std::printf(__VA_ARGS__); std::printf("\n"); } } } while(0)

static int asInt(float f) { int i; std::memcpy(&i, &f, 4); return i; }
static uint32_t bitsOf(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char **argv)
{
	if(argc < 3) { std::printf("usage: flat_table_check MESH LEAF_SIZE\n"); return 2; }
	FILE *f = std::fopen(argv[1], "rb");
	if(!f) { std::printf("cannot open %s\n", argv[1]); return 2; }
	int nv = 0, nt = 0;
	if(std::fread(&nv, 4, 1, f) != 1 || std::fread(&nt, 4, 1, f) != 1 || nv <= 0 || nt <= 0) { std::printf("bad header\n"); return 2; }
	std::vector<float> verts(3 * (size_t)nv);
	std::vector<int> tris(3 * (size_t)nt);
	if(std::fread(verts.data(), 4, verts.size(), f) != verts.size() || std::fread(tris.data(), 4, tris.size(), f) != tris.size()) { std::printf("short file\n"); return 2; }
	std::fclose(f);
	BvhInput in{verts.data(), tris.data(), nt};
	const BvhOutput b = buildBvh(in, std::atoi(argv[2]), 1);
	CHECK(b.width == 4, "not a BVH4");
	const FlatTable t = buildFlatTable(b.nodes.data(), b.n_nodes);

	// the tree's own leaves, by first slot
	struct Leaf { int node, k, first, count; };
	std::vector<Leaf> leaves;
	int past = 0;
	for(int node = 0; node < b.n_nodes; ++node)
		for(int k = 0; k < 4; ++k)
		{
			const float *o = &b.nodes[32 * (size_t)node];
			const int c = asInt(o[24 + k]), cnt = asInt(o[28 + k]);
			if(c >= 0 || cnt <= 0) continue;
			leaves.push_back({node, k, ~c, cnt});
			if(~c + cnt > kFlatMaxTris) ++past;
		}
	if(nt > kFlatMaxTris)
	{
		// a tree with slots past 63 has no table, and no leaf count makes it eligible
		CHECK(past > 0 && t.n == 0 && t.rec.empty(), "%d triangles: a table of %d records", nt, t.n);
		CHECK(!flatEligible(nt, 1, true) && !flatEligible(nt, 1, false), "%d triangles are eligible", nt);
		std::printf("%d triangles, %zu leaves: no table\n", nt, leaves.size());
		return fails ? 1 : 0;
	}
	CHECK(t.n == (int)leaves.size(), "L = %d, the tree has %zu leaves", t.n, leaves.size());
	CHECK((int)t.rec.size() == t.n + 1, "%zu records for L = %d", t.rec.size(), t.n);
	CHECK(0 <= t.n_lo && t.n_lo <= t.n_mid && t.n_mid <= t.n, "ranges %d %d %d", t.n_lo, t.n_mid, t.n);
	CHECK(flatPack(t) == (t.n | (t.n_lo << 8) | (t.n_mid << 16)), "flatPack");
	uint64_t seen = 0;
	int prev_first = -1;
	for(int i = 0; i < t.n && i < (int)t.rec.size(); ++i)
	{
		const FlatLeaf &r = t.rec[i];
		const uint64_t bits = ((uint64_t)r.bits_hi << 32) | r.bits_lo;
		CHECK(bits != 0, "record %d: no slot", i);
		CHECK((seen & bits) == 0, "record %d: a slot twice", i);
		seen |= bits;
		const int first = __builtin_ctzll(bits | (1ull << 63)), count = __builtin_popcountll(bits);
		CHECK(first > prev_first, "record %d: not ordered by first slot", i);
		prev_first = first;
		CHECK(bits == ((count == 64 ? ~0ull : (1ull << count) - 1ull) << first), "record %d: slots not contiguous", i);
		// its leaf in the tree: the same slots, the same box bits
		const Leaf *l = nullptr;
		for(const Leaf &c : leaves) if(c.first == first) l = &c;
		CHECK(l && l->count == count, "record %d: no leaf [%d, %d) in the tree", i, first, first + count);
		if(l)
		{
			const float *o = &b.nodes[32 * (size_t)l->node];
			for(int a = 0; a < 3; ++a)
				CHECK(bitsOf(r.lo[a]) == bitsOf(o[8 * a + l->k]) && bitsOf(r.hi[a]) == bitsOf(o[8 * a + 4 + l->k]), "record %d axis %d: box bits differ from node %d child %d", i,
				      a, l->node, l->k);
		}
		// the word range the scan puts it in
		const int words = (r.bits_lo ? 1 : 0) | (r.bits_hi ? 2 : 0);
		CHECK(words == (i < t.n_lo ? 1 : i < t.n_mid ? 3 : 2), "record %d: words %d in the wrong range (%d %d)", i, words, t.n_lo, t.n_mid);
	}
	CHECK(seen == (nt == 64 ? ~0ull : (1ull << nt) - 1ull), "slots covered %016llx of %d triangles", (unsigned long long)seen, nt);
	if(!t.rec.empty())
	{
		const FlatLeaf z{};
		CHECK(std::memcmp(&t.rec.back(), &z, sizeof(z)) == 0, "the spare record is not zero");
	}
	static_assert(sizeof(FlatLeaf) == 32, "one record = one 32-byte scalar load");
	// eligibility
	CHECK(flatEligible(nt, t.n, true), "forced: not eligible");
	CHECK(flatEligible(nt, t.n, false) == (t.n <= kFlatMaxLeaves), "automatic: L = %d against the limit %d", t.n, kFlatMaxLeaves);
	CHECK(!flatEligible(65, 10, true) && !flatEligible(65, 10, false), "65 triangles are eligible");
	CHECK(flatEligible(64, kFlatMaxLeaves, false) && !flatEligible(64, kFlatMaxLeaves + 1, false), "the automatic limit");
	CHECK(flatEligible(64, 64, true) && !flatEligible(64, 65, true), "the forced limit");
	CHECK(!flatEligible(0, 0, true), "an empty scene is eligible");
	std::printf("%d triangles, L = %d (%d / %d / %d by mask word), largest leaf %d\n", nt, t.n, t.n_lo, t.n_mid - t.n_lo, t.n - t.n_mid, b.max_leaf);
	return fails ? 1 : 0;
}
