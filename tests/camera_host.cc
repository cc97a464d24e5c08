// Host build of the camera numerics: devmath.h's libm restatements beside the host's own libm, and the ray
// functions of the orthographic, equirectangular and angular cameras (the top of libyafaray_amd/csrc/camera.h, the
// exact code the kernels run), with extern "C" wrappers for tests/test_cameras_host.py.  Compiled with
// g++ -ffp-contract=off at test time.
#include "../libyafaray_amd/csrc/camera.h"
#include <cmath>
using namespace yafamd;
extern "C" {
// which 0: asinf, 1: atanf, 2: math::asin's clamp around asinf
void ch_libm(int which, const float *x, int n, float *dev, float *libm)
{
	for(int i = 0; i < n; ++i)
	{
		if(which == 0) { dev[i] = libmAsinf(x[i]); libm[i] = ::asinf(x[i]); }
		else if(which == 1) { dev[i] = libmAtanf(x[i]); libm[i] = ::atanf(x[i]); }
		else
		{
			dev[i] = mathAsin(x[i]);
			libm[i] = x[i] <= -1.f ? -1.57079637f : x[i] >= 1.f ? 1.57079637f : ::asinf(x[i]);
		}
	}
}
// frame: vright, vup, vto (9 floats); pos 3 floats; pxy: n (px, py) pairs; out: n (from, dir) of 6 floats
void ch_ortho(const float *frame, const float *pos, const float *pxy, int n, float *out)
{
	const V3 vr = v3(frame[0], frame[1], frame[2]), vu = v3(frame[3], frame[4], frame[5]), vt = v3(frame[6], frame[7], frame[8]);
	for(int i = 0; i < n; ++i)
	{
		V3 from, dir;
		orthoRay(v3(pos[0], pos[1], pos[2]), vr, vu, vt, pxy[2 * i], pxy[2 * i + 1], from, dir);
		out[6 * i] = from.x; out[6 * i + 1] = from.y; out[6 * i + 2] = from.z;
		out[6 * i + 3] = dir.x; out[6 * i + 4] = dir.y; out[6 * i + 5] = dir.z;
	}
}
void ch_equirect(const float *frame, int resx, int resy, const float *pxy, int n, float *out)
{
	const V3 vr = v3(frame[0], frame[1], frame[2]), vu = v3(frame[3], frame[4], frame[5]), vt = v3(frame[6], frame[7], frame[8]);
	for(int i = 0; i < n; ++i)
	{
		const V3 d = equirectDir(vr, vu, vt, resx, resy, pxy[2 * i], pxy[2 * i + 1]);
		out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
	}
}
// valid[i]: 1 when the camera gives the sample a ray
void ch_angular(const float *frame, int resx, int resy, float aspect_ratio, float focal_length, float max_radius, int circular, int projection,
                const float *pxy, int n, float *out, int *valid)
{
	const V3 vr = v3(frame[0], frame[1], frame[2]), vu = v3(frame[3], frame[4], frame[5]), vt = v3(frame[6], frame[7], frame[8]);
	for(int i = 0; i < n; ++i)
	{
		V3 d = v3(0.f, 0.f, 0.f);
		valid[i] = angularDir(vr, vu, vt, resx, resy, aspect_ratio, focal_length, max_radius, circular, projection, pxy[2 * i], pxy[2 * i + 1], d) ? 1 : 0;
		out[3 * i] = d.x; out[3 * i + 1] = d.y; out[3 * i + 2] = d.z;
	}
}
}
