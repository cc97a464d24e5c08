// Render layers ("Render layers"): the first-hit layers of a render that defines any — z-depth-abs,
// z-depth-norm, mist, debug-normal-geom, debug-normal-smooth, debug-uv, debug-barycentric-uvw,
// adv-diffuse-color and the absolute / normalised object and material index layers.
//
// Each of them is a closed-form function of the camera ray's first intersection
// (TiledIntegrator::generateCommonLayers, integrator_tiled.cc:410-630, and the per-sample rules of
// renderTile, :362-403), so none of it is threaded through the wavefront: a pass of its own regenerates
// every sample's camera ray (camera.h sampleAt / cameraRay, the render's own rays bit for bit), finds the
// closest hit with the exact traversal (trace.h), and keeps a 16-byte record per sample; k_layer_film then
// splats every defined layer from the records with k_film's arithmetic (filmmath.h) in k_film's order.
//
// A translation unit of its own: everything it shares with the path tracer and the film is device-inline code in
// headers, so the build needs no relocatable device code for it.
//
// The first-hit pass and the depth pre-pass keep the whole traversal stack in LDS (k_trace_rays'
// context: stack bound x block x 4 bytes, no spill column); render.cc refuses the layers of a BVH
// whose bound exceeds 64 KB of it instead of launching.
#include <hip/hip_runtime.h>
#include "devmath.h"
#include "devscene.h"
#include "trace.h"
#include "texeval.h"
#include "camera.h"
#include "filmmath.h"
#include "launch.h"

namespace yafamd
{

// ---------------------------------------------------------------------------------------------
// depth range (TiledIntegrator::precalcDepths, integrator_tiled.cc:69-95)
// ---------------------------------------------------------------------------------------------
// The closest hit of one ray with the whole stack in LDS (k_trace_rays' context).
template<bool WIDE>
__device__ __forceinline__ bool layerClosest(const DevScene &S, float4 *smem, int stack_depth, V3 o, V3 d, float tmin, float tmax, float &t, int &prim)
{
	TraceCtx C;
	C.wave_base = waveBase();
	C.stack = reinterpret_cast<int *>(smem);
	C.lds_depth = stack_depth;   // the full bound: no spill
	C.spill = nullptr;
	C.spill_stride = 0;
	C.nodes = S.nodes;
	C.tris = S.tris;
	uint32_t visits = 0, tests = 0;
	return traverse<false, WIDE, false>(C, o, d, tmin, tmax, t, prim, visits, tests);
}

// One ray per camera pixel through shootRay(i, j, 0.5, 0.5) as the reference calls it — the row index
// as x and the column index as y, no half-pixel offset — then max_depth_ = the largest tmax and
// min_depth_ = the smallest non-negative one (a miss keeps the camera's tmax).  Non-negative floats
// order like their bits, so the wave's extremes go to two integer atomics.  range: (min, max) bits,
// started at (1e38f, 0.f).
// CAMX: the orthographic, equirectangular and angular cameras (camera.h shootRayX).  The reference takes no notice of
// a ray the camera did not set up, so the render refuses the circular angular camera before this pass (render.cc).
template<bool WIDE, bool CAMX = false>
__global__ void __launch_bounds__(kTraceBlock) k_layer_depth(DevScene S, uint32_t *range, int stack_depth)
{
	extern __shared__ float4 smem[];
	const DevCamera &c = S.cam;
	const int w = c.resx, h = c.resy;
	const int k = blockIdx.x * blockDim.x + threadIdx.x;
	float tm = -1.f;
	if(k < w * h)
	{
		const float px = (float)(k / w), py = (float)(k % w);
		V3 from, dir;
		float tmin, tmax;
		bool valid = true;
		if constexpr(CAMX) valid = shootRayX(c, px, py, from, dir, tmin, tmax);
		else
		{
			const V3 pos = v3(c.pos[0], c.pos[1], c.pos[2]);
			dir = v3(c.vright[0], c.vright[1], c.vright[2]) * px + v3(c.vup[0], c.vup[1], c.vup[2]) * py + v3(c.vto[0], c.vto[1], c.vto[2]);
			dir = normalize(dir);
			const V3 cz = v3(c.cam_z[0], c.cam_z[1], c.cam_z[2]);
			tmin = dot(cz, v3(c.near_p[0], c.near_p[1], c.near_p[2]) - pos) / dot(dir, cz);
			tmax = dot(cz, v3(c.far_p[0], c.far_p[1], c.far_p[2]) - pos) / dot(dir, cz);
			from = pos;
			if(c.aperture != 0.f)
			{
				float u, v;
				lensUv(c, 0.5f, 0.5f, u, v);
				const V3 li = v3(c.dof_rt[0], c.dof_rt[1], c.dof_rt[2]) * u + v3(c.dof_up[0], c.dof_up[1], c.dof_up[2]) * v;
				from = from + li;
				dir = normalize(dir * c.dof_distance - li);
			}
		}
		// (CAMX: a pixel without a ray takes no part; the render refuses such a camera before this pass)
		if(valid)
		{
			float t;
			int prim;
			const bool hit = layerClosest<WIDE>(S, smem, stack_depth, from, dir, c.ray_tt ? tmin : 0.f,
			                                    (c.ray_tt && tmax >= 0.f) ? tmax : __builtin_huge_valf(), t, prim);
			tm = hit ? t : tmax;
		}
	}
	// (tmax > max_depth_ with max_depth_ >= 0; tmax < min_depth_ && tmax >= 0: a NaN takes part in neither)
	uint32_t hi = (tm > 0.f) ? __float_as_uint(tm) : 0u;
	uint32_t lo = (tm >= 0.f) ? __float_as_uint(tm == 0.f ? 0.f : tm) : 0xffffffffu;
	for(int off = 32; off > 0; off >>= 1)
	{
		hi = max(hi, (uint32_t)__shfl_down(hi, off));
		lo = min(lo, (uint32_t)__shfl_down(lo, off));
	}
	if((threadIdx.x & 63u) == 0)
	{
		if(lo < range[0]) atomicMin(&range[0], lo);
		if(hi > range[1]) atomicMax(&range[1], hi);
	}
}

// "we use the inverse multiplicative of the value aquired" (integrator_tiled.cc:94)
__global__ void k_layer_depth_fin(float *range)
{
	if(blockIdx.x == 0 && threadIdx.x == 0 && range[1] > 0.f) range[1] = 1.f / (range[1] - range[0]);
}

// ---------------------------------------------------------------------------------------------
// first hits
// ---------------------------------------------------------------------------------------------
constexpr int kLayerNoRay = -2;   // the record's primitive of a sample the camera gave no ray (-1: a miss)
// material_shiny_diffuse.cc:662-666 getDiffuseColor (every other material: Material's black)
__device__ __forceinline__ C3 layerDiffuseColor(const DevScene &S, int prim, V3 o, V3 d, float t)
{
	const DevMaterial &m = S.mats[__float_as_int(S.prim_ng[prim].w)];
	if(m.type != MAT_SHINYDIFFUSE || !(m.sd_flags & SD_DIFFUSE)) return C3{0.f, 0.f, 0.f};
	C3 dcol = C3{m.diffuse[0], m.diffuse[1], m.diffuse[2]};
	float drefl = 1.f, sigma = 0.f;
	if(m.n_nodes > 0 && S.has_attr)
	{
		const V3 p = o + t * d;   // accelerator.cc:61
		const SurfAttr sa = surfAttr(S.prim_attr, S.prim_ng, prim, o, d, p);
		evalNodes(m, S.shader_nodes, S.textures, S.texels, sa, dcol, drefl, sigma);
	}
	const float k = (m.n_nodes > 0 && m.drefl_root >= 0) ? drefl : m.comp[3];
	return C3{k * dcol.r, k * dcol.g, k * dcol.b};
}

// CAMX: the cameras of cameraRayX; a sample without a ray leaves the record (-1, kLayerNoRay): every layer's default colour
template<bool WIDE, bool CAMX = false>
__global__ void __launch_bounds__(kTraceBlock) k_layer_hits(DevScene S, DevLayers L, const DevJob *jobs, int n_jobs, uint64_t chunk_base, int n,
                                                            int stack_depth)
{
	extern __shared__ float4 smem[];
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if(i >= n) return;
	const SampleCoord sc = sampleAt(S, jobs, n_jobs, chunk_base + (uint64_t)i);
	V3 from, dir;
	float tmin, tmax;
	uint32_t seed;
	if constexpr(CAMX)
	{
		if(!cameraRayX(S, sc, from, dir, tmin, tmax, seed))
		{
			const size_t at = ((size_t)sc.y * S.width + sc.x) * S.spp + sc.s;
			L.rec[at] = make_float4(-1.f, __int_as_float(kLayerNoRay), 0.f, 0.f);
			if(L.albedo) L.albedo[at] = make_float4(0.f, 0.f, 0.f, 1.f);
			return;
		}
	}
	else cameraRay(S, sc, from, dir, tmin, tmax, seed);
	// (k_camera / k_trace: without ray_tt every camera ray has (0, unbounded))
	float t;
	int prim;
	const bool hit = layerClosest<WIDE>(S, smem, stack_depth, from, dir, S.cam.ray_tt ? tmin : 0.f,
	                                    (S.cam.ray_tt && tmax >= 0.f) ? tmax : __builtin_huge_valf(), t, prim);
	float u = 0.f, v = 0.f;
	if(hit && L.prim_attr)
	{
		// primitive_triangle.cc:44-71: the barycentrics of the hit (texeval.h surfAttr's operations)
		const float4 *a = L.prim_attr + (size_t)prim * kAttrF4;
		const V3 v0 = xyz4(a[0]), e1 = xyz4(a[1]), e2 = xyz4(a[2]);
		const V3 pvec = cross(dir, e2);
		const float det = dot(e1, pvec);
		const float inv_det = 1.f / det;
		const V3 tvec = from - v0;
		u = dot(tvec, pvec) * inv_det;
		const V3 qvec = cross(tvec, e1);
		v = dot(dir, qvec) * inv_det;
	}
	const size_t at = ((size_t)sc.y * S.width + sc.x) * S.spp + sc.s;
	L.rec[at] = make_float4(hit ? t : tmax, __int_as_float(hit ? prim : -1), u, v);
	if(L.albedo)
	{
		const C3 c = hit ? layerDiffuseColor(S, prim, from, dir, t) : C3{0.f, 0.f, 0.f};
		L.albedo[at] = make_float4(c.r, c.g, c.b, 1.f);
	}
}

// ---------------------------------------------------------------------------------------------
// layer values + film
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float4 layerGray(float g) { return make_float4(g, g, g, g > 1.f ? 1.f : g); }   // Rgba{float}: alpha = g, clamped (:386)
__device__ __forceinline__ float4 layerNormal(V3 n) { return make_float4((n.x + 1.f) * .5f, (n.y + 1.f) * .5f, (n.z + 1.f) * .5f, 1.f); }

// One layer's colour of one sample (generateCommonLayers + integrator_tiled.cc:383-400)
__device__ __forceinline__ float4 layerValue(int kind, const DevLayers &L, const float4 *prim_ng, const float4 &rec, const float4 *albedo_at)
{
	const float t = rec.x;
	const int prim = __float_as_int(rec.y);
	if(kind == LK_ZDEPTH_ABS || kind == LK_ZDEPTH_NORM || kind == LK_MIST)
	{
		if(prim == kLayerNoRay) return make_float4(0.f, 0.f, 0.f, 1.f);   // no camera ray: LayerDef's default colour
		if(t < 0.f) return make_float4(0.f, 0.f, 0.f, 0.f);   // background: fully transparent
		if(kind == LK_ZDEPTH_ABS) return layerGray(t);
		const float mn = L.depth[0], mx = L.depth[1];
		if(kind == LK_ZDEPTH_NORM) return layerGray(1.f - (t - mn) * mx);
		return layerGray((t - mn) * mx);
	}
	if((uint32_t)prim >= (uint32_t)L.n_prims) return make_float4(0.f, 0.f, 0.f, 1.f);   // a miss: LayerDef's default colour
	const float bu = 1.f - rec.z - rec.w, bv = rec.z, bw = rec.w;
	switch(kind)
	{
		case LK_BARYCENTRIC: return make_float4(bu, bv, bw, 1.f);
		case LK_UV:
		{
			const float4 *a = L.prim_attr + (size_t)prim * kAttrF4;
			if(__float_as_uint(a[0].w) & ATTR_UV)
			{
				const float4 uv01 = a[6], uv2 = a[7];
				return make_float4(bu * uv01.x + bv * uv01.z + bw * uv2.x, bu * uv01.y + bv * uv01.w + bw * uv2.y, 0.f, 1.f);
			}
			return make_float4(bu, bv, 0.f, 1.f);
		}
		case LK_NORMAL_GEOM: return layerNormal(xyz4(prim_ng[prim]));
		case LK_NORMAL_SMOOTH:
		{
			const float4 *a = L.prim_attr + (size_t)prim * kAttrF4;
			if(__float_as_uint(a[0].w) & ATTR_SMOOTH) return layerNormal(normalize(bu * xyz4(a[8]) + bv * xyz4(a[9]) + bw * xyz4(a[10])));
			return layerNormal(xyz4(prim_ng[prim]));
		}
		case LK_DIFFUSE_COLOR: return *albedo_at;
		case LK_MAT_INDEX_ABS:
		case LK_MAT_INDEX_NORM:
		{
			const uint32_t mat = (uint32_t)__float_as_int(prim_ng[prim].w);
			float g = mat < (uint32_t)L.n_mats ? L.mat_index[mat] : 0.f;
			if(kind == LK_MAT_INDEX_NORM) g = g / L.mat_highest;
			return make_float4(g, g, g, 1.f);
		}
		default:   // LK_OBJ_INDEX_ABS / LK_OBJ_INDEX_NORM: the last object whose first primitive is <= prim
		{
			int lo = 0, hi = L.n_obj_seg - 1;
			while(lo < hi)
			{
				const int mid = (lo + hi + 1) >> 1;
				if(L.obj_seg[mid].x <= prim) lo = mid;
				else hi = mid - 1;
			}
			float g = (float)(uint32_t)L.obj_seg[lo].y;
			if(kind == LK_OBJ_INDEX_NORM) g = g / L.obj_highest;
			return make_float4(g, g, g, 1.f);
		}
	}
}

// k_film for the layer planes: the same candidate order, footprints, table weights, clamp and
// normalisation; every sample's weight is computed once and every defined layer accumulates
// v * wt from the sample's record.  accum / out: L.n planes of W x H float4, in kind order.  The
// weights are only read (k_film, launched after this kernel with the same arguments, writes them).
template<int RF, int RB>
__global__ void __launch_bounds__(256) k_layer_film(DevFilm F, DevLayers L, const float4 *prim_ng, const uint8_t *flags, float4 *accum, float4 *out,
                                                    const float *weights, int y0, int y1, float clamp_samples, int accumulate)
{
	constexpr bool kStatic = RF >= 0;
	constexpr int kWin = kStatic ? (RF + RB + 1) * (RF + RB + 1) : 81;
	const int x = blockIdx.x * blockDim.x + threadIdx.x;
	const int y = y0 + blockIdx.y;
	if(x >= F.width || y >= y1) return;
	const int W = F.width, H = F.height, spp = F.spp;
	const int rf = kStatic ? RF : F.reach_fwd, rb = kStatic ? RB : F.reach_back;
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
			if(F.partial && tileRankOf(F, xx, yy) > own_tile) continue;
			const uint64_t r = pixelRank(F, xx, yy, W, H, F.tile);
			int p = n++;
			while(p > 0 && rk[p - 1] > r) { rk[p] = rk[p - 1]; sx[p] = sx[p - 1]; sy[p] = sy[p - 1]; --p; }
			rk[p] = r; sx[p] = xx; sy[p] = yy;
		}
	}
	const size_t p = (size_t)y * W + x, plane = (size_t)W * H;
	float wsum = accumulate ? weights[p] : 0.f;
	float4 acc[LK_COUNT];
#pragma unroll
	for(int l = 0; l < LK_COUNT; ++l)
		acc[l] = (accumulate && l < L.n) ? accum[(size_t)l * plane + p] : make_float4(0.f, 0.f, 0.f, 0.f);
	const float d_1 = 1.f / (float)spp;
	for(int c = 0; c < n; ++c)
	{
		const int px = sx[c], py = sy[c];
		const uint32_t offset = fnv32((uint32_t)(py + F.crop_y0) * fnv32((uint32_t)(px + F.crop_x0)));
		const int ox = x - px, oy = y - py;
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
			const int dx_0 = max(0 - px, roundToInt((double)dx - F.filterw));
			const int dx_1 = min(W - px - 1, roundToInt((double)dx + F.filterw - 1.0));
			const int dy_0 = max(0 - py, roundToInt((double)dy - F.filterw));
			const int dy_1 = min(H - py - 1, roundToInt((double)dy + F.filterw - 1.0));
			if(ox < dx_0 || ox > dx_1 || oy < dy_0 || oy > dy_1) continue;
			const int xi = floorToInt(fabs(((double)ox - (dx - 0.5)) * F.table_scale));
			const int yi = floorToInt(fabs(((double)oy - (dy - 0.5)) * F.table_scale));
			const float wt = F.table[yi * 16 + xi];
			wsum = wsum + wt;
			const size_t at = ((size_t)py * W + px) * spp + s;
			const float4 rec = L.rec[at];
#pragma unroll
			for(int l = 0; l < LK_COUNT; ++l)
			{
				if(l >= L.n) continue;
				const float4 col = layerValue(L.kind[l], L, prim_ng, rec, L.albedo ? L.albedo + at : nullptr);
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
				acc[l].x = acc[l].x + r * wt;
				acc[l].y = acc[l].y + g * wt;
				acc[l].z = acc[l].z + b * wt;
				acc[l].w = acc[l].w + col.w * wt;
			}
		}
	}
	const float inv = wsum != 0.f ? 1.f / wsum : 0.f;
#pragma unroll
	for(int l = 0; l < LK_COUNT; ++l)
	{
		if(l >= L.n) continue;
		if(!F.partial) accum[(size_t)l * plane + p] = acc[l];
		out[(size_t)l * plane + p] = wsum != 0.f ? make_float4(acc[l].x * inv, acc[l].y * inv, acc[l].z * inv, acc[l].w * inv)
		                                         : make_float4(0.f, 0.f, 0.f, 0.f);
	}
}

} // namespace yafamd

using namespace yafamd;

extern "C" {

// precalcDepths over the camera's resx x resy pixel rays; range: 2 floats on the device
hipError_t yafamd_layer_depth_range(const DevScene *S, float *range, int stack_depth, hipStream_t st)
{
	const float init[2] = {1e38f, 0.f};
	hipError_t e = hipMemcpyAsync(range, init, sizeof(init), hipMemcpyHostToDevice, st);
	if(e != hipSuccess) return e;
	e = hipStreamSynchronize(st);   // `init` leaves scope
	if(e != hipSuccess) return e;
	const int n = S->cam.resx * S->cam.resy;
	if(n > 0)
	{
		const size_t stack_bytes = (size_t)stack_depth * kTraceBlock * sizeof(int);
		const dim3 grid((n + kTraceBlock - 1) / kTraceBlock);
		const bool camx = S->cam.kind != CAM_PERSPECTIVE;
		if(camx && S->node_f4 == 8) hipLaunchKernelGGL((k_layer_depth<true, true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, (uint32_t *)range, stack_depth);
		else if(camx) hipLaunchKernelGGL((k_layer_depth<false, true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, (uint32_t *)range, stack_depth);
		else if(S->node_f4 == 8) hipLaunchKernelGGL((k_layer_depth<true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, (uint32_t *)range, stack_depth);
		else hipLaunchKernelGGL((k_layer_depth<false>), grid, dim3(kTraceBlock), stack_bytes, st, *S, (uint32_t *)range, stack_depth);
		e = hipGetLastError();
		if(e != hipSuccess) return e;
	}
	hipLaunchKernelGGL(k_layer_depth_fin, dim3(1), dim3(64), 0, st, range);
	return hipGetLastError();
}

hipError_t yafamd_launch_layer_hits(const DevScene *S, const DevLayers *L, const DevJob *jobs, int n_jobs, uint64_t chunk_base, int n, int stack_depth,
                                    hipStream_t st)
{
	if(n <= 0) return hipSuccess;
	const size_t stack_bytes = (size_t)stack_depth * kTraceBlock * sizeof(int);
	const dim3 grid((n + kTraceBlock - 1) / kTraceBlock);
	const bool camx = S->cam.kind != CAM_PERSPECTIVE;
	if(camx && S->node_f4 == 8) hipLaunchKernelGGL((k_layer_hits<true, true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, *L, jobs, n_jobs, chunk_base, n, stack_depth);
	else if(camx) hipLaunchKernelGGL((k_layer_hits<false, true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, *L, jobs, n_jobs, chunk_base, n, stack_depth);
	else if(S->node_f4 == 8) hipLaunchKernelGGL((k_layer_hits<true>), grid, dim3(kTraceBlock), stack_bytes, st, *S, *L, jobs, n_jobs, chunk_base, n, stack_depth);
	else hipLaunchKernelGGL((k_layer_hits<false>), grid, dim3(kTraceBlock), stack_bytes, st, *S, *L, jobs, n_jobs, chunk_base, n, stack_depth);
	return hipGetLastError();
}

hipError_t yafamd_launch_layer_film(const DevFilm *F, const DevLayers *L, const float4 *prim_ng, const uint8_t *flags, float4 *accum, float4 *out,
                                    const float *weights, int y0, int y1, float clamp_samples, int accumulate, hipStream_t st)
{
	if(y1 <= y0 || L->n <= 0) return hipSuccess;
	const dim3 grid((F->width + 255) / 256, y1 - y0);
	if(F->reach_fwd == 1 && F->reach_back == 0)
		hipLaunchKernelGGL((k_layer_film<1, 0>), grid, dim3(256), 0, st, *F, *L, prim_ng, flags, accum, out, weights, y0, y1, clamp_samples, accumulate);
	else
		hipLaunchKernelGGL((k_layer_film<-1, -1>), grid, dim3(256), 0, st, *F, *L, prim_ng, flags, accum, out, weights, y0, y1, clamp_samples,
		                   accumulate);
	return hipGetLastError();
}

}
