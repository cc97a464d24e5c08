// Object instances, expanded on the device into the flat world-space arrays the renderer consumes.
//
// Reference: an ObjectInstance wraps every primitive of its base object in a PrimitiveInstance that
// hands obj_to_world to the base triangle (primitive_instance.cc:28-66); all of them go into the one
// flat accelerator (scene.cc:1032-1060), and the triangle works on transformed vertices
// (primitive_face.cc:31-36, primitive_triangle.cc:39-41).  So an instance is a per-primitive
// expansion: the host uploads each base's object-space rows once plus a table of segments
// (DevInstSeg), these kernels write `verts`, `tris`, `prim_ng` and `prim_attr` for every segment.
// A visible plain mesh is an identity segment: its rows are copied, no arithmetic touches them.
//
// The rules, all in float and in the expression order of matrix4.h:78-90 (-ffp-contract=off):
//   vertex            M * Point3: m[i][0] x + m[i][1] y + m[i][2] z + m[i][3]
//   geometric normal  normalize(M * ng_base), the Vec3 product (no translation, no inverse transpose),
//                     ng_base = the base triangle's normalize((b - a) ^ (c - a)) (primitive_face.cc:130-134)
//   vertex normals    normalize(M * n); a vertex without a normal gets the instance's geometric
//                     normal (primitive_face.cc:44-53)
//   orco              the base's, untransformed; without orco the orco normal is ng_base
//                     (primitive_triangle.cc:114-127), kept in attribute row 3 (ATTR_BASE_NG)
//   uv, material      carried over
//   dPdU / dPdV       edges of the transformed vertices (primitive_triangle.cc:129-158)
#include <hip/hip_runtime.h>
#include <cstdint>

#include "devmath.h"
#include "devscene.h"
#include "launch.h"

namespace
{
using namespace yafamd;

constexpr int kB = 256;

// the last segment whose first output vertex (or primitive) is <= i; the host emits no empty segment
__device__ __forceinline__ int findSeg(const DevInstSeg *segs, int n, int i, bool prim)
{
	int lo = 0, hi = n - 1;
	while(lo < hi)
	{
		const int mid = (lo + hi + 1) >> 1;
		const int first = prim ? segs[mid].out_prim0 : segs[mid].out_vert0;
		if(first <= i) lo = mid;
		else hi = mid - 1;
	}
	return lo;
}

__device__ __forceinline__ V3 ld3(const float *v, int k) { return v3(v[3 * (size_t)k], v[3 * (size_t)k + 1], v[3 * (size_t)k + 2]); }
__device__ __forceinline__ V3 xyz(float4 a) { return v3(a.x, a.y, a.z); }
__device__ __forceinline__ float4 f4(V3 a, float w) { return make_float4(a.x, a.y, a.z, w); }

// matrix4.h:85-90
__device__ __forceinline__ V3 mulPoint(const float *m, V3 b)
{
	return v3(m[0] * b.x + m[1] * b.y + m[2] * b.z + m[3], m[4] * b.x + m[5] * b.y + m[6] * b.z + m[7], m[8] * b.x + m[9] * b.y + m[10] * b.z + m[11]);
}

// matrix4.h:78-83
__device__ __forceinline__ V3 mulVec(const float *m, V3 b)
{
	return v3(m[0] * b.x + m[1] * b.y + m[2] * b.z, m[4] * b.x + m[5] * b.y + m[6] * b.z, m[8] * b.x + m[9] * b.y + m[10] * b.z);
}

// one thread per output vertex; per-workgroup partial bound of the written positions
__global__ void __launch_bounds__(kB) k_instance_expand_verts(const DevInstSeg *segs, int n_segs, const float *src_verts, int n, float *out_verts,
                                                              float *partial)
{
	const int i = blockIdx.x * kB + threadIdx.x;
	float c[3] = {3.4e38f, 3.4e38f, 3.4e38f}, d[3] = {-3.4e38f, -3.4e38f, -3.4e38f};
	if(i < n)
	{
		const DevInstSeg &g = segs[findSeg(segs, n_segs, i, false)];
		V3 p = ld3(src_verts, g.src_vert0 + (i - g.out_vert0));
		if(!g.identity) p = mulPoint(g.m, p);
		out_verts[3 * (size_t)i] = p.x;
		out_verts[3 * (size_t)i + 1] = p.y;
		out_verts[3 * (size_t)i + 2] = p.z;
		c[0] = d[0] = p.x;
		c[1] = d[1] = p.y;
		c[2] = d[2] = p.z;
	}
	__shared__ float red[6][kB];
	for(int k = 0; k < 3; ++k) { red[k][threadIdx.x] = c[k]; red[3 + k][threadIdx.x] = d[k]; }
	__syncthreads();
	for(int w = kB / 2; w > 0; w >>= 1)
	{
		if(threadIdx.x < w)
			for(int k = 0; k < 3; ++k)
			{
				red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + w]);
				red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + w]);
			}
		__syncthreads();
	}
	if(threadIdx.x < 6) partial[6 * (size_t)blockIdx.x + threadIdx.x] = red[threadIdx.x][0];
}

// the scene bound: the partial bounds of g workgroups folded by one (lo xyz, hi xyz)
__global__ void __launch_bounds__(kB) k_instance_bounds(const float *partial, int g, float *bounds)
{
	float v[6] = {3.4e38f, 3.4e38f, 3.4e38f, -3.4e38f, -3.4e38f, -3.4e38f};
	for(int b = threadIdx.x; b < g; b += kB)
		for(int k = 0; k < 3; ++k)
		{
			v[k] = fminf(v[k], partial[6 * (size_t)b + k]);
			v[3 + k] = fmaxf(v[3 + k], partial[6 * (size_t)b + 3 + k]);
		}
	__shared__ float red[6][kB];
	for(int k = 0; k < 6; ++k) red[k][threadIdx.x] = v[k];
	__syncthreads();
	for(int w = kB / 2; w > 0; w >>= 1)
	{
		if(threadIdx.x < w)
			for(int k = 0; k < 3; ++k)
			{
				red[k][threadIdx.x] = fminf(red[k][threadIdx.x], red[k][threadIdx.x + w]);
				red[3 + k][threadIdx.x] = fmaxf(red[3 + k][threadIdx.x], red[3 + k][threadIdx.x + w]);
			}
		__syncthreads();
	}
	if(threadIdx.x < 6) bounds[threadIdx.x] = red[threadIdx.x][0];
}

// one thread per output primitive: its vertex indices and the geometric normal row (.w = material)
__global__ void __launch_bounds__(kB) k_instance_expand(const DevInstSeg *segs, int n_segs, const int *src_tris, const float4 *src_ng, int n,
                                                        int *out_tris, float4 *out_ng)
{
	const int i = blockIdx.x * kB + threadIdx.x;
	if(i >= n) return;
	const DevInstSeg &g = segs[findSeg(segs, n_segs, i, true)];
	const size_t sp = (size_t)g.src_prim0 + (size_t)(i - g.out_prim0);
	out_tris[3 * (size_t)i] = g.out_vert0 + src_tris[3 * sp];
	out_tris[3 * (size_t)i + 1] = g.out_vert0 + src_tris[3 * sp + 1];
	out_tris[3 * (size_t)i + 2] = g.out_vert0 + src_tris[3 * sp + 2];
	float4 ng = src_ng[sp];
	if(!g.identity) ng = f4(normalize(mulVec(g.m, xyz(ng))), ng.w);
	out_ng[i] = ng;
}

// one thread per float4 of the output attribute rows (devscene.h: kAttrF4 per primitive), so that a
// wavefront loads and stores consecutive float4
__global__ void __launch_bounds__(kB) k_instance_expand_attr(const DevInstSeg *segs, int n_segs, const float *src_verts, const int *src_tris,
                                                             const float4 *src_ng, const float4 *src_attr, int n, float4 *out_attr)
{
	const size_t j = (size_t)blockIdx.x * kB + threadIdx.x;
	if(j >= (size_t)n * kAttrF4) return;
	const int i = (int)(j / kAttrF4), r = (int)(j % kAttrF4);
	const DevInstSeg &g = segs[findSeg(segs, n_segs, i, true)];
	const size_t sp = (size_t)g.src_prim0 + (size_t)(i - g.out_prim0);
	const float4 *sa = src_attr + sp * kAttrF4;
	float4 v = sa[r];
	const uint32_t fl = __float_as_uint(r == 0 ? v.w : sa[0].w);
	if(r == 0)
	{
		uint32_t o = fl & ~ATTR_SRC_MASK;
		if(!g.identity)
		{
			if(!(fl & ATTR_ORCO)) o |= ATTR_BASE_NG;
			v = f4(mulPoint(g.m, xyz(v)), 0.f);
		}
		v.w = __uint_as_float(o);
	}
	else if(g.identity) {}
	else if(r <= 2)
	{
		const V3 p0 = mulPoint(g.m, ld3(src_verts, g.src_vert0 + src_tris[3 * sp]));
		const V3 p1 = mulPoint(g.m, ld3(src_verts, g.src_vert0 + src_tris[3 * sp + r]));
		v = f4(p1 - p0, v.w);
	}
	else if(r == 3)
	{
		if(!(fl & ATTR_ORCO)) v = f4(xyz(src_ng[sp]), 0.f);
	}
	else if(r >= 8 && (fl & ATTR_SMOOTH))
	{
		const V3 nb = (fl & (ATTR_SRC_FACE_N0 << (r - 8))) ? xyz(src_ng[sp]) : xyz(v);
		v = f4(normalize(mulVec(g.m, nb)), v.w);
	}
	out_attr[j] = v;
}

inline int blocks(size_t n) { return (int)((n + kB - 1) / kB); }

} // namespace

// Everything on the device.  segs: n_segs segments in output order; src_*: the object-space rows
// (src_attr / out_attr may be null: no surface attributes); out_verts: 3 n_out_verts floats, out_tris:
// 3 n_out_prims indices into them, out_ng: n_out_prims float4, out_attr: kAttrF4 n_out_prims float4;
// bounds: 6 floats (lo xyz, hi xyz of the written vertices).  Returns after the stream drained.
extern "C" hipError_t yafamd_instance_expand(const yafamd::DevInstSeg *segs, int n_segs, const float *src_verts, const int *src_tris,
                                             const float4 *src_ng, const float4 *src_attr, int n_out_verts, int n_out_prims, float *out_verts,
                                             int *out_tris, float4 *out_ng, float4 *out_attr, float *bounds, hipStream_t st)
{
	const int g = n_segs > 0 && n_out_verts > 0 ? blocks((size_t)n_out_verts) : 0;
	float *partial = nullptr;
	hipError_t e = hipMalloc(&partial, (size_t)(g > 0 ? g : 1) * 6 * sizeof(float));
	if(e != hipSuccess) return e;
	if(g > 0) hipLaunchKernelGGL(k_instance_expand_verts, dim3(g), dim3(kB), 0, st, segs, n_segs, src_verts, n_out_verts, out_verts, partial);
	hipLaunchKernelGGL(k_instance_bounds, dim3(1), dim3(kB), 0, st, partial, g, bounds);
	if(n_segs > 0 && n_out_prims > 0)
	{
		hipLaunchKernelGGL(k_instance_expand, dim3(blocks((size_t)n_out_prims)), dim3(kB), 0, st, segs, n_segs, src_tris, src_ng, n_out_prims, out_tris,
		                   out_ng);
		if(src_attr && out_attr)
			hipLaunchKernelGGL(k_instance_expand_attr, dim3(blocks((size_t)n_out_prims * kAttrF4)), dim3(kB), 0, st, segs, n_segs, src_verts, src_tris,
			                   src_ng, src_attr, n_out_prims, out_attr);
	}
	e = hipGetLastError();
	const hipError_t es = hipStreamSynchronize(st);
	(void)hipFree(partial);
	return e != hipSuccess ? e : es;
}
