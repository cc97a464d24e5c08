// Sample coordinates and camera rays: sample id -> pixel and sample index (sampleCoord over the jobs, sampleAt
// with an adaptive pass's pixel list), the lens functions, and cameraRay (the sample position of
// TiledIntegrator::renderTile and PerspectiveCamera::shootRay).  Used by k_camera, the camera-stage k_shade and
// k_path and k_gather's sample write (kernels.hip), k_done_flags (film.hip) and the render layers (layers.hip),
// which regenerate the render's own camera rays bit for bit.  Device-inline code only, but for the rays of the
// orthographic, equirectangular and angular cameras at the top: those are YD functions of plain vectors and scalars,
// which a host program compiles without the HIP headers (tests/camera_host.cc).
#pragma once

#include <cstdint>
#include "devmath.h"
#include "camkind.h"

namespace yafamd
{

// plane.h:37-40 with the camera's planes (normal cam_z): the ray's own from
YD void cameraClip(V3 cam_z, V3 near_p, V3 far_p, V3 from, V3 dir, float &tmin, float &tmax)
{
	tmin = dot(cam_z, near_p - from) / dot(dir, cam_z);
	tmax = dot(cam_z, far_p - from) / dot(dir, cam_z);
}

// camera_orthographic.cc:52-59: pos is pos_, vright / vup carry scale / res, the direction is cam_z as it stands
YD void orthoRay(V3 pos, V3 vright, V3 vup, V3 vto, float px, float py, V3 &from, V3 &dir)
{
	from = pos + vright * px + vup * py;
	dir = vto;
}

// camera_equirectangular.cc:48-60: phi and theta are long double products rounded to float; not normalised
YD V3 equirectDir(V3 vright, V3 vup, V3 vto, int resx, int resy, float px, float py)
{
	const float u = 2.f * px / (float)resx - 1.f;
	const float v = 2.f * py / (float)resy - 1.f;
	const float phi = x87mul(kPi, u);
	const float theta = x87mul(kDivPiBy2, v);
	return fcos(theta) * (fcos(phi) * vto + fsin(phi) * vright) + fsin(theta) * vup;
}

// camera_angular.cc:58-78: false for a sample outside the circle (an invalid sample: no ray)
YD bool angularDir(V3 vright, V3 vup, V3 vto, int resx, int resy, float aspect_ratio, float focal_length, float max_radius,
                   int circular, int projection, float px, float py, V3 &dir)
{
	const float u = 1.f - 2.f * (px / (float)resx);
	float v = 2.f * (py / (float)resy) - 1.f;
	v *= aspect_ratio;
	const float radius = sqrtf(u * u + v * v);
	if(circular && radius > max_radius) return false;
	float theta = 0.f;
	if(!((u == 0.f) && (v == 0.f))) theta = libmAtan2f(v, u);
	float phi;
	if(projection == AP_ORTHOGRAPHIC) phi = mathAsin(radius / focal_length);
	else if(projection == AP_STEREOGRAPHIC) phi = 2.f * libmAtanf(radius / (2.f * focal_length));
	else if(projection == AP_EQUISOLID) phi = 2.f * mathAsin(radius / (2.f * focal_length));
	else if(projection == AP_RECTILINEAR) phi = libmAtanf(radius / focal_length);
	else phi = radius / focal_length;
	dir = fsin(phi) * (fcos(theta) * vright + fsin(theta) * vup) + fcos(phi) * vto;
	return true;
}

} // namespace yafamd

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#include "devscene.h"

namespace yafamd
{

struct SampleCoord { int x, y, s; };

// (sampleCoord and lensUv are plain __device__ definitions, as they were in kernels.hip: without relocatable device
// code every unit's code object gets a copy of its own and none reaches the host.  `inline` would be the form for an
// -fgpu-rdc build; it also raises the inliner's threshold, so it is left out to keep the generated code.)
// sample id (frame-local enumeration over jobs) -> pixel + sample index
__device__ SampleCoord sampleCoord(const DevJob *jobs, int n_jobs, int width, int tile, int spp, uint64_t sid)
{
	// last job whose first sample is <= sid (jobs are in ascending sample_base order)
	int j = 0, hi = n_jobs - 1;
	while(j < hi)
	{
		const int mid = (j + hi + 1) >> 1;
		if(jobs[mid].sample_base <= sid) j = mid;
		else hi = mid - 1;
	}
	const DevJob job = jobs[j];
	const uint64_t local = sid - job.sample_base;
	const uint32_t pix = (uint32_t)(local / (uint64_t)spp);
	const int s = (int)(local % (uint64_t)spp);
	const int bh = job.y1 - job.y0;
	const uint32_t per_tile = (uint32_t)(tile * bh);
	const int tx = (int)(pix / per_tile);
	const int tw = min(tile, width - tx * tile);
	const uint32_t l = pix - (uint32_t)tx * per_tile;
	SampleCoord c;
	c.x = tx * tile + (int)(l % (uint32_t)tw);
	c.y = job.y0 + (int)(l / (uint32_t)tw);
	c.s = s;
	return c;
}

// camera_perspective.cc:71-85
__device__ __forceinline__ float biasDist(int bias, float r)
{
	if(bias == 1) return sqrtf(sqrtf(r) * r);           // BbCenter
	if(bias == 2) return sqrtf(1.f - r * r);            // BbEdge
	return sqrtf(r);                                    // BbNone
}

// vector.cc:128-163 (the long double pi/4 products round like x87)
__device__ __forceinline__ void shirleyDisk(float r_1, float r_2, float &u, float &v)
{
	float phi = 0.f, r = 0.f;
	const float a = 2.f * r_1 - 1.f, b = 2.f * r_2 - 1.f;
	if(a > -b)
	{
		if(a > b) { r = a; phi = x87mul(kDivPiBy4, b / a); }
		else { r = b; phi = x87mul(kDivPiBy4, 2.f - a / b); }
	}
	else
	{
		if(a < b) { r = -a; phi = x87mul(kDivPiBy4, 4.f + b / a); }
		else
		{
			r = -b;
			phi = (b != 0) ? x87mul(kDivPiBy4, 6.f - a / b) : 0.f;
		}
	}
	u = r * fcos(phi);
	v = r * fsin(phi);
}

// camera_perspective.cc:87-124 getLensUv (sampleTsd for the polygon bokehs)
__device__ void lensUv(const DevCamera &c, float r_1, float r_2, float &u, float &v)
{
	const int t = c.bokeh_type;
	if(t >= 3 && t <= 6)
	{
		const float fn = static_cast<float>(t);
		int idx = int(r_1 * fn);
		r_1 = (r_1 - ((float)idx) / fn) * fn;
		r_1 = biasDist(c.bokeh_bias, r_1);
		const float b_1 = r_1 * r_2;
		const float b_0 = r_1 - b_1;
		idx <<= 1;
		u = c.ls[idx] * b_0 + c.ls[idx + 2] * b_1;
		v = c.ls[idx + 1] * b_0 + c.ls[idx + 3] * b_1;
	}
	else if(t == 1 || t == 7)
	{
		const float w = 6.28318548f * r_2;   // (float)math::mult_pi_by_2 * r_2
		if(t == 7) r_1 = sqrtf((float)0.707106781 + (float)0.292893218);
		else r_1 = biasDist(c.bokeh_bias, r_1);
		u = r_1 * fcos(w);
		v = r_1 * fsin(w);
	}
	else shirleyDisk(r_1, r_2, u, v);
}

// sample id -> pixel + sample index: the jobs' enumeration, or an adaptive pass's pixel list
__device__ __forceinline__ SampleCoord sampleAt(const DevScene &S, const DevJob *jobs, int n_jobs, uint64_t sid)
{
	if(S.plist)
	{
		const uint32_t pix = S.plist[sid / (uint64_t)S.spp];
		SampleCoord c;
		c.x = (int)(pix % (uint32_t)S.width);
		c.y = (int)(pix / (uint32_t)S.width);
		c.s = (int)(sid % (uint64_t)S.spp);
		return c;
	}
	return sampleCoord(jobs, n_jobs, S.width, S.tile, S.spp, sid);
}

// The sample's position in camera pixels (integrator_tiled.cc:313-335; a cropped film starts at crop_x0 / crop_y0)
// and the offset of its pixel's sampling sequences
__device__ __forceinline__ void samplePos(const DevScene &S, const SampleCoord &sc, float &px, float &py, uint32_t &offset)
{
	const int cx = sc.x + S.crop_x0, cy = sc.y + S.crop_y0;
	offset = fnv32((uint32_t)cy * fnv32((uint32_t)cx));
	const uint32_t sample_idx = S.base_offset + S.pass_offset + (uint32_t)sc.s;   // PixelSamplingData::sample_
	float dx = 0.5f, dy = 0.5f;
	if(S.aa_multipass)
	{
		dx = riVdC(sample_idx, offset);
		dy = riS(sample_idx, offset);
	}
	else if(S.spp > 1)
	{
		const float d_1 = 1.f / (float)S.spp;
		dx = (0.5f + (float)sc.s) * d_1;
		dy = riLp((uint32_t)sc.s + offset);
	}
	px = (float)cx + dx;
	py = (float)cy + dy;
}

// RR generator: per-sample MWC (the reference seeds one per tile from rand(), so RR
// output is matched statistically — integrator_tiled.cc:272), seeded from the pixel-major sample
// id so that the image does not depend on how the film is split over GPUs or chunks
// (64-bit id: W * H * spp passes 2^32 at 4K x 1024 spp; both halves are hashed)
__device__ __forceinline__ uint32_t sampleSeed(const DevScene &S, const SampleCoord &sc)
{
	const uint64_t gid = ((uint64_t)sc.y * (uint64_t)S.width + (uint64_t)sc.x) * (uint64_t)S.spp + (uint64_t)sc.s;
	const uint32_t gid32 = (uint32_t)gid ^ fnv32((uint32_t)(gid >> 32));
	return fnv32(gid32 ^ S.rr_seed ^ (S.pass_offset * 0x9e3779b9u)) + 123u;
}

// One camera sample: TiledIntegrator::renderTile's sample position (integrator_tiled.cc:313-340) and
// PerspectiveCamera::shootRay (camera_perspective.cc:128-146), plus the sample's Russian-roulette seed.
// k_camera (wavefront) and k_path (megakernel) both start their samples here.
__device__ __forceinline__ void cameraRay(const DevScene &S, const SampleCoord &sc, V3 &from, V3 &dir, float &tmin, float &tmax, uint32_t &seed)
{
	float px, py;
	uint32_t offset;
	samplePos(S, sc, px, py, offset);
	// camera_perspective.cc:128-146, plane.h:37-40
	const DevCamera &c = S.cam;
	const V3 pos = v3(c.pos[0], c.pos[1], c.pos[2]);
	dir = v3(c.vright[0], c.vright[1], c.vright[2]) * px + v3(c.vup[0], c.vup[1], c.vup[2]) * py + v3(c.vto[0], c.vto[1], c.vto[2]);
	dir = normalize(dir);
	const V3 cz = v3(c.cam_z[0], c.cam_z[1], c.cam_z[2]);
	tmin = dot(cz, v3(c.near_p[0], c.near_p[1], c.near_p[2]) - pos) / dot(dir, cz);
	tmax = dot(cz, v3(c.far_p[0], c.far_p[1], c.far_p[2]) - pos) / dot(dir, cz);
	from = pos;
	if(c.aperture != 0.f)
	{
		// integrator_tiled.cc:314-316, 336-340: Halton(3) / Halton(5) lens streams started at the
		// pass offset + pixel offset, one getNext() per sample; camera_perspective.cc:137-144
		const uint32_t hstart = S.base_offset + S.pass_offset + offset;
		const float lu = haltonNext(3u, hstart, sc.s + 1), lv = haltonNext(5u, hstart, sc.s + 1);
		float u, v;
		lensUv(c, lu, lv, u, v);
		const V3 li = v3(c.dof_rt[0], c.dof_rt[1], c.dof_rt[2]) * u + v3(c.dof_up[0], c.dof_up[1], c.dof_up[2]) * v;
		from = from + li;
		dir = normalize(dir * c.dof_distance - li);
	}
	seed = sampleSeed(S, sc);
}

// shootRay of the orthographic, equirectangular and angular cameras (DevCamera::kind != CAM_PERSPECTIVE) at camera
// pixel position (px, py): false for a sample the camera gives no ray (angular, outside the circle)
__device__ __forceinline__ bool shootRayX(const DevCamera &c, float px, float py, V3 &from, V3 &dir, float &tmin, float &tmax)
{
	const V3 vright = v3(c.vright[0], c.vright[1], c.vright[2]), vup = v3(c.vup[0], c.vup[1], c.vup[2]), vto = v3(c.vto[0], c.vto[1], c.vto[2]);
	from = v3(c.pos[0], c.pos[1], c.pos[2]);
	bool valid = true;
	if(c.kind == CAM_ORTHO) orthoRay(from, vright, vup, vto, px, py, from, dir);
	else if(c.kind == CAM_EQUIRECT) dir = equirectDir(vright, vup, vto, c.resx, c.resy, px, py);
	else valid = angularDir(vright, vup, vto, c.resx, c.resy, c.aspect_ratio, c.focal_length, c.max_radius, c.circular, c.projection, px, py, dir);
	if(valid)
		cameraClip(v3(c.cam_z[0], c.cam_z[1], c.cam_z[2]), v3(c.near_p[0], c.near_p[1], c.near_p[2]), v3(c.far_p[0], c.far_p[1], c.far_p[2]),
		           from, dir, tmin, tmax);
	return valid;
}

// cameraRay with those cameras: the CAMX instantiations of k_camera and k_layer_hits, launched for them alone.
// These cameras have no lens, so no lens sample is drawn.
__device__ __forceinline__ bool cameraRayX(const DevScene &S, const SampleCoord &sc, V3 &from, V3 &dir, float &tmin, float &tmax, uint32_t &seed)
{
	float px, py;
	uint32_t offset;
	samplePos(S, sc, px, py, offset);
	seed = sampleSeed(S, sc);
	return shootRayX(S.cam, px, py, from, dir, tmin, tmax);
}

} // namespace yafamd
#endif // __HIPCC__
