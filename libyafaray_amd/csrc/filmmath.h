// The film arithmetic k_film (film.hip) and k_layer_film (layers.hip) share: the reference's integer rounding and
// the rank of a pixel in the single-thread tile order.  Device-inline code only.
#pragma once

#include <hip/hip_runtime.h>
#include <cstdint>
#include "devscene.h"

namespace yafamd
{

__device__ __forceinline__ int roundToInt(double v) { return (int)(v + (.5 - 1.4e-11)); }
__device__ __forceinline__ int floorToInt(double v) { return (int)floor(v); }

// rank of a pixel in the single-thread tile order (imagesplitter.cc:30-107): tiles by their rank
// (linear when F.tile_rank is null), pixels row-major inside a tile (integrator_tiled.cc:288-290)
__device__ __forceinline__ uint32_t tileRankOf(const DevFilm &F, int x, int y)
{
	const int ty = y / F.tile, tx = x / F.tile;
	return F.tile_rank ? F.tile_rank[ty * F.ntx + tx] : (uint32_t)(ty * F.ntx + tx);
}
__device__ __forceinline__ uint64_t pixelRank(const DevFilm &F, int x, int y, int W, int H, int ts)
{
	const int ty = y / ts, tx = x / ts;
	const int tw = min(ts, W - tx * ts);
	return (uint64_t)tileRankOf(F, x, y) * (uint64_t)ts * ts + (uint64_t)(y - ty * ts) * tw + (x - tx * ts);
}

} // namespace yafamd
