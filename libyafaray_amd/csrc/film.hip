// The film kernels: k_film (ImageFilm::addSample, imagefilm.cc:680-733, as a per-destination-pixel gather that
// replays the reference's single-thread linear-tile splat order, so every film sum is bit-identical without a mutex
// or atomics; then the flush normalisation, imagefilm.cc:590-617, color.h:554-558), k_done_flags (the pixels a
// canceled render completed) and the light-pick counter sums k_lpc_seg / k_lpc_prefix, with their launch wrappers.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devscene.h"
#include "camera.h"
#include "filmmath.h"
#include "launch.h"

namespace yafamd
{

// ---------------------------------------------------------------------------------------------
// k_film: deterministic gather splat + flush normalisation
// ---------------------------------------------------------------------------------------------

// RF / RB: compile-time footprint reach (box and gauss filters: RF = 1, RB = 0 -> a 2x2 window
// kept in registers); RF = RB = -1 selects the generic runtime window (<= 9x9).
template<int RF, int RB>
__global__ void __launch_bounds__(256) k_film(DevFilm F, const float4 *samples, const uint8_t *flags, float4 *accum,
                                              float4 *out, float *weights, int y0, int y1, float clamp_samples, int accumulate)
{
	constexpr bool kStatic = RF >= 0;
	constexpr int kWin = kStatic ? (RF + RB + 1) * (RF + RB + 1) : 81;
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = y0 + blockIdx.y;
	if(x >= F.width || y >= y1) return;
	const int W = F.width, H = F.height, spp = F.spp;
	const int rf = kStatic ? RF : F.reach_fwd, rb = kStatic ? RB : F.reach_back;
	// candidate sources, sorted by their rank in the reference's splat order
	int sx[kWin], sy[kWin];
	uint64_t rk[kWin];
	int n = 0;
	const uint32_t own_tile = F.partial ? tileRankOf(F, x, y) : 0u;
#pragma unroll
	for(int dyy = 0; dyy < (kStatic ? RF + RB + 1 : 9); ++dyy)
	{
#pragma unroll
		for(int dxx = 0; dxx < (kStatic ? RF + RB + 1 : 9); ++dxx)
		{
			if(!kStatic && (dyy > rf + rb || dxx > rf + rb)) continue;
			const int yy = y - rf + dyy, xx = x - rf + dxx;
			if(yy < 0 || yy >= H || xx < 0 || xx >= W) continue;
			if(F.partial && tileRankOf(F, xx, yy) > own_tile) continue;   // tile not finished yet
			const uint64_t r = pixelRank(F, xx, yy, W, H, F.tile);
			int p = n++;
			while(p > 0 && rk[p - 1] > r) { rk[p] = rk[p - 1]; sx[p] = sx[p - 1]; sy[p] = sy[p - 1]; --p; }
			rk[p] = r; sx[p] = xx; sy[p] = yy;
		}
	}
	const size_t p = (size_t)y * W + x;
	// adaptive passes add to the film of the earlier passes (imagefilm.cc addSample: += per sample)
	float wsum = accumulate ? weights[p] : 0.f;
	float4 acc = accumulate ? accum[p] : make_float4(0.f, 0.f, 0.f, 0.f);
	const float d_1 = 1.f / (float)spp;
	for(int c = 0; c < n; ++c)
	{
		const int px = sx[c], py = sy[c];
		const uint32_t offset = fnv32((uint32_t)(py + F.crop_y0) * fnv32((uint32_t)(px + F.crop_x0)));
		const int ox = x - px, oy = y - py;
		// adaptive pass: only resampled pixels splat.  (Skipping them while building the candidate list
		// instead lost diagonal candidates in the unrolled k_film<1, 0> — tools/film_probe.hip.)
		const int ns = (flags && !flags[(size_t)py * W + px]) ? 0 : spp;
		for(int s = 0; s < ns; ++s)
		{
			float dx = 0.5f, dy = 0.5f;
			if(F.multipass)
			{
				dx = riVdC(F.sample_offset + (uint32_t)s, offset);
				dy = riS(F.sample_offset + (uint32_t)s, offset);
			}
			else if(spp > 1)
			{
				dx = (0.5f + (float)s) * d_1;
				dy = riLp((uint32_t)s + offset);
			}
			// imagefilm.cc:684-707 footprint of this sample, then the table weight at (x, y)
			const int dx_0 = max(0 - px, roundToInt((double)dx - F.filterw));
			const int dx_1 = min(W - px - 1, roundToInt((double)dx + F.filterw - 1.0));
			const int dy_0 = max(0 - py, roundToInt((double)dy - F.filterw));
			const int dy_1 = min(H - py - 1, roundToInt((double)dy + F.filterw - 1.0));
			if(ox < dx_0 || ox > dx_1 || oy < dy_0 || oy > dy_1) continue;
			const int xi = floorToInt(fabs(((double)ox - (dx - 0.5)) * F.table_scale));
			const int yi = floorToInt(fabs(((double)oy - (dy - 0.5)) * F.table_scale));
			const float wt = F.table[yi * 16 + xi];
			wsum = wsum + wt;
			const float4 col = samples[((size_t)py * W + px) * spp + s];
			float r = col.x, g = col.y, b = col.z;
			if(clamp_samples > 0.f)
			{
				// color.h:415-440 clampProportionalRgb
				const float max_rgb = fmaxf(r, fmaxf(g, b));
				const float adj = clamp_samples / max_rgb;
				if(max_rgb > clamp_samples)
				{
					if(r >= max_rgb) { r = clamp_samples; g *= adj; b *= adj; }
					else if(g >= max_rgb) { g = clamp_samples; r *= adj; b *= adj; }
					else { b = clamp_samples; r *= adj; g *= adj; }
				}
			}
			acc.x = acc.x + r * wt;
			acc.y = acc.y + g * wt;
			acc.z = acc.z + b * wt;
			acc.w = acc.w + col.w * wt;
		}
	}
	if(!F.partial)
	{
		weights[p] = wsum;
		accum[p] = acc;
	}
	// Rgba::normalized (color.h:554-558): colour * (1 / weight) — operator/ takes the reciprocal first
	if(wsum != 0.f)
	{
		const float inv = 1.f / wsum;
		out[p] = make_float4(acc.x * inv, acc.y * inv, acc.z * inv, acc.w * inv);
	}
	else out[p] = make_float4(0.f, 0.f, 0.f, 0.f);
}

// Canceled render (integrator_tiled.cc:292: a canceled worker stops before its next pixel, so a
// pixel is either fully sampled or not at all): flags the pixels whose samples the completed
// chunks rendered, for k_film's `flags` argument.  Pass 0 enumerates the jobs (pixel ranks
// [0, n_pix)); an adaptive pass (plist) clears the flags of its pixels beyond `done_pix`.
__global__ void __launch_bounds__(256) k_done_flags(DevScene S, const DevJob *jobs, int n_jobs, uint32_t n_pix, uint32_t done_pix,
                                                    uint8_t *flags)
{
	const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
	if(p >= n_pix) return;
	if(S.plist)
	{
		if(p >= done_pix) flags[S.plist[p]] = 0;
		return;
	}
	const SampleCoord c = sampleCoord(jobs, n_jobs, S.width, S.tile, S.spp, (uint64_t)p * (uint64_t)S.spp);
	flags[(size_t)c.y * S.width + c.x] = p < done_pix ? 1 : 0;
}

// ---------------------------------------------------------------------------------------------
// light-pick counters (DevScene::lpc, render.cc lpcBases).  A row segment = one row of one tile: its
// pixels' counters (spp each) are contiguous in the pixel-major layout, and the one-thread render
// visits them in that order (renderTile, integrator_tiled.cc:281-345: rows, then pixels, then
// samples).  k_lpc_seg sums each segment of rows [y0, y1); k_lpc_prefix turns each segment's
// counts into the counter values its samples start from: the segment's base (the calls of every
// sample visited before the segment, from the host) + the exclusive prefix sum inside it.
// One wave per segment.
// ---------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_lpc_seg(const uint32_t *lpc, int W, int spp, int ts, int y0, int y1, uint32_t *seg)
{
	const int ntx = (W + ts - 1) / ts;
	const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / 64u), lane = (int)(threadIdx.x & 63u);
	if(wave >= (y1 - y0) * ntx) return;
	const int y = y0 + wave / ntx, tx = wave % ntx;
	const int x0 = tx * ts, x1 = min(W, x0 + ts);
	const size_t b = ((size_t)y * W + x0) * spp, n = (size_t)(x1 - x0) * spp;
	uint32_t acc = 0;
	for(size_t k = lane; k < n; k += 64) acc += lpc[b + k];
	for(int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off);
	if(lane == 0) seg[(size_t)y * ntx + tx] = acc;
}

__global__ void __launch_bounds__(256) k_lpc_prefix(uint32_t *lpc, int W, int spp, int ts, int y0, int y1, const uint32_t *segbase)
{
	const int ntx = (W + ts - 1) / ts;
	const int wave = (int)((blockIdx.x * blockDim.x + threadIdx.x) / 64u), lane = (int)(threadIdx.x & 63u);
	if(wave >= (y1 - y0) * ntx) return;
	const int y = y0 + wave / ntx, tx = wave % ntx;
	const int x0 = tx * ts, x1 = min(W, x0 + ts);
	const size_t b = ((size_t)y * W + x0) * spp, n = (size_t)(x1 - x0) * spp;
	uint32_t carry = segbase[(size_t)y * ntx + tx];
	for(size_t k0 = 0; k0 < n; k0 += 64)
	{
		const size_t k = k0 + (size_t)lane;
		const uint32_t v = k < n ? lpc[b + k] : 0u;
		uint32_t x = v;
		for(int off = 1; off < 64; off <<= 1)
		{
			const uint32_t t = __shfl_up(x, off);
			if(lane >= off) x += t;
		}
		if(k < n) lpc[b + k] = carry + (x - v);
		carry += __shfl(x, 63);
	}
}

} // namespace yafamd

using namespace yafamd;

extern "C" {

hipError_t yafamd_launch_done_flags(const DevScene *S, const DevJob *jobs, int n_jobs, uint32_t n_pix, uint32_t done_pix, uint8_t *flags,
                                    hipStream_t st)
{
	if(n_pix == 0) return hipSuccess;
	hipLaunchKernelGGL(k_done_flags, dim3((n_pix + 255) / 256), dim3(256), 0, st, *S, jobs, n_jobs, n_pix, done_pix, flags);
	return hipGetLastError();
}

hipError_t yafamd_lpc_seg(const uint32_t *lpc, int W, int spp, int ts, int y0, int y1, uint32_t *seg, hipStream_t st)
{
	const int n = (y1 - y0) * ((W + ts - 1) / ts);
	if(n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_lpc_seg, dim3((n + 3) / 4), dim3(256), 0, st, lpc, W, spp, ts, y0, y1, seg);
	return hipGetLastError();
}

hipError_t yafamd_lpc_prefix(uint32_t *lpc, int W, int spp, int ts, int y0, int y1, const uint32_t *segbase, hipStream_t st)
{
	const int n = (y1 - y0) * ((W + ts - 1) / ts);
	if(n <= 0) return hipSuccess;
	hipLaunchKernelGGL(k_lpc_prefix, dim3((n + 3) / 4), dim3(256), 0, st, lpc, W, spp, ts, y0, y1, segbase);
	return hipGetLastError();
}

hipError_t yafamd_launch_film(const DevFilm *F, const float4 *samples, const uint8_t *flags, float4 *accum, float4 *out,
                              float *weights, int y0, int y1, float clamp_samples, int accumulate, hipStream_t st)
{
	if(y1 <= y0) return hipSuccess;
	const dim3 grid((F->width + 255) / 256, y1 - y0);
	if(F->reach_fwd == 1 && F->reach_back == 0)
		hipLaunchKernelGGL((k_film<1, 0>), grid, dim3(256), 0, st, *F, samples, flags, accum, out, weights, y0, y1, clamp_samples, accumulate);
	else
		hipLaunchKernelGGL((k_film<-1, -1>), grid, dim3(256), 0, st, *F, samples, flags, accum, out, weights, y0, y1, clamp_samples,
		                   accumulate);
	return hipGetLastError();
}

}
