// Device build of the hot path's numerics (libyafaray_amd/csrc/devmath.h and texeval.h) for tests/test_devmath_gpu.py:
// one plain kernel per function family (one work-item per input, global loads and stores, bounds-checked) behind an
// extern "C" wrapper that takes host pointers, so the test can compare what gfx950 computes with the g++ build of the
// same header (tests/devmath_host.cc, whose entry points these mirror), with the golden vectors, and, for texeval.h,
// which g++ cannot build, with the host pass of this very translation unit.  Built by `make devcheck` with the product's
// device flags; never part of libyafaray4.so.
#include "../libyafaray_amd/csrc/devmath.h"
#include "../libyafaray_amd/csrc/texeval.h"

#include <vector>

using namespace yafamd;

namespace
{
constexpr int kBlock = 256;

YD X87Const constOf(int c)
{
	switch(c)
	{
		case 0: return kPi;
		case 1: return kDivPiBy2;
		case 2: return kDiv1ByPi;
		case 3: return kMultPiBy2;
		case 4: return kDiv1By2Pi;
		case 5: return kDiv4ByPi;
		default: return kDiv4BySquaredPi;
	}
}

// Device buffers of one wrapper call: every size comes from the caller's n, the first HIP error is kept and
// returned, and nothing is launched once there is one.
struct Call
{
	int err = 0;
	std::vector<void *> bufs;
	void ck(hipError_t e) { if(!err && e != hipSuccess) err = (int)e; }
	template<class T> T *out(size_t n)
	{
		void *d = nullptr;
		if(err) return nullptr;
		ck(hipMalloc(&d, (n ? n : 1) * sizeof(T)));
		if(err) return nullptr;
		bufs.push_back(d);
		return static_cast<T *>(d);
	}
	template<class T> T *in(const T *h, size_t n)
	{
		T *d = out<T>(n);
		if(d && n) ck(hipMemcpy(d, h, n * sizeof(T), hipMemcpyHostToDevice));
		return d;
	}
	bool ready(int n) const { return !err && n > 0; }
	dim3 grid(int n) const { return dim3((unsigned)((n + kBlock - 1) / kBlock)); }
	void ran()
	{
		ck(hipGetLastError());
		ck(hipDeviceSynchronize());
	}
	template<class T> void back(T *h, const T *d, size_t n)
	{
		if(!err && n) ck(hipMemcpy(h, d, n * sizeof(T), hipMemcpyDeviceToHost));
	}
	int done()
	{
		for(void *p : bufs)
		{
			const hipError_t e = hipFree(p);
			ck(e);
		}
		bufs.clear();
		return err;
	}
};

// ---- x87 emulation ----
__global__ void k_round(const double *hi, const double *lo, int n, double *r_hi, double *r_lo, float *r24)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const DD r = round64(DD{hi[i], lo[i]});
	r_hi[i] = r.hi;
	r_lo[i] = r.lo;
	r24[i] = round24(r);
}
__global__ void k_x87mul(int c, const float *x, float *disp, float *exact, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const X87Const k = constOf(c);
	disp[i] = x87mul(k, x[i]);
	exact[i] = x87mulExact(k.hi, k.lo, x[i]);
}
__global__ void k_x87mul2(int c, const float *x, const float *y, float *disp, float *exact, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const X87Const k = constOf(c);
	disp[i] = x87mul2(k, x[i], y[i]);
	exact[i] = x87mul2Exact(k.hi, k.lo, x[i], y[i]);
}
__global__ void k_x87mul3(int c, const float *x, const float *y, const float *z, float *disp, float *exact, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const X87Const k = constOf(c);
	disp[i] = x87mul3(k, x[i], y[i], z[i]);
	exact[i] = x87mul3Exact(k.hi, k.lo, x[i], y[i], z[i]);
}
__global__ void k_x87muldiv(int c, const float *a, const float *b, float *disp, float *exact, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const X87Const k = constOf(c);
	disp[i] = x87mulDiv(k, a[i], b[i]);
	exact[i] = x87mulDivExact(k.hi, k.lo, a[i], b[i]);
}
__global__ void k_x87recip(int c, const float *a, float *disp, float *exact, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const X87Const k = constOf(c);
	disp[i] = x87recipMul(k, a[i]);
	exact[i] = x87recipMulExact(k.hi, k.lo, a[i]);
}
__global__ void k_x87one_minus(int c, const float *x, float *disp, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	disp[i] = x87oneMinus2Mul(constOf(c), x[i]);
}

// ---- libm restatements ----
__global__ void k_libm(const float *y, const float *x, int n, float *o_atan2, float *o_acos, float *o_asin, float *o_atan,
                       float *o_masin)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o_atan2[i] = libmAtan2f(y[i], x[i]);
	o_acos[i] = libmAcosf(y[i]);
	o_asin[i] = libmAsinf(y[i]);
	o_atan[i] = libmAtanf(y[i]);
	o_masin[i] = mathAsin(y[i]);
}

// ---- FAST_TRIG, vectors ----
__global__ void k_sincos(const float *x, float *o_sin, float *o_cos, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o_sin[i] = fsin(x[i]);
	o_cos[i] = fcos(x[i]);
}
__global__ void k_hemi(const float *p, const float *s, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const float *q = p + 9 * (size_t)i;
	const V3 r = cosHemisphere(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]), s[2 * (size_t)i], s[2 * (size_t)i + 1]);
	o[3 * (size_t)i] = r.x; o[3 * (size_t)i + 1] = r.y; o[3 * (size_t)i + 2] = r.z;
}
__global__ void k_coords(const float *in, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	V3 u, v;
	coordsSystem(v3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]), u, v);
	float *q = o + 6 * (size_t)i;
	q[0] = u.x; q[1] = u.y; q[2] = u.z; q[3] = v.x; q[4] = v.y; q[5] = v.z;
}
__global__ void k_normalize(const float *in, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	const V3 r = normalize(v3(in[3 * (size_t)i], in[3 * (size_t)i + 1], in[3 * (size_t)i + 2]));
	o[3 * (size_t)i] = r.x; o[3 * (size_t)i + 1] = r.y; o[3 * (size_t)i + 2] = r.z;
}

// ---- samplers ----
__global__ void k_ri(int which, const uint32_t *b, const uint32_t *r, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o[i] = which == 0 ? riVdC(b[i], r[i]) : which == 1 ? riS(b[i], r[i]) : riLp(b[i], r[i]);
}
__global__ void k_fnv(const uint32_t *in, uint32_t *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o[i] = fnv32(in[i]);
}
__global__ void k_bitrev(const uint32_t *in, uint32_t *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o[i] = bitReverse32(in[i]);
}
__global__ void k_udiv(uint32_t d, const uint32_t *in, uint32_t *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o[i] = udiv(in[i], udivMake(d));
}
__global__ void k_lds(const uint8_t *perm, uint32_t base, double f, const uint32_t *idx, double *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	o[i] = lowDiscrepancy(perm, base, udivMake(base), f, idx[i]);
}
// one work-item per seed, `steps` draws each
__global__ void k_mwc(const uint32_t *seed, int steps, double *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	Mwc m{30903u, seed[i]};
	for(int j = 0; j < steps; ++j) o[(size_t)i * steps + j] = m.next();
}
template<uint32_t B>
__device__ void haltonIncRun(uint32_t start, int k, float *o)
{
	HaltonInc<B> h;
	h.start(start);
	for(int j = 0; j < k; ++j) o[j] = h.next();
}
__global__ void k_halton(uint32_t base, const uint32_t *start, int n, int k, float *first, float *next, float *inc)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i >= n) return;
	first[i] = haltonFirst(base, 1.0 / (double)base, start[i]);
	for(int j = 0; j < k; ++j) next[(size_t)i * k + j] = haltonNext(base, start[i], j + 1);
	float *o = inc + (size_t)i * k;
	if(base == 2) haltonIncRun<2>(start[i], k, o);
	else if(base == 3) haltonIncRun<3>(start[i], k, o);
	else if(base == 5) haltonIncRun<5>(start[i], k, o);
}

// ---- texeval.h: each body once, run by the kernel and by the wrapper's host pass ----
YD float texPow(const float *ab, int i) { return fmPow(ab[2 * (size_t)i], ab[2 * (size_t)i + 1]); }
YD void texColorSpace(int cs, float gamma, const float *rgb, float *o, int i)
{
	const float *p = rgb + 3 * (size_t)i;
	const C4 c = colorSpaceFromLinear(c4(p[0], p[1], p[2], 1.f), cs, gamma);
	o[3 * (size_t)i] = c.r; o[3 * (size_t)i + 1] = c.g; o[3 * (size_t)i + 2] = c.b;
}
// rgbToHsv, the scale-and-wrap step, hsvToRgb as applyColorAdjust does it (texture.cc:230-240)
YD void texHsv(const float *rgb, const float *sat_hue, float *o, int i)
{
	const float *p = rgb + 3 * (size_t)i;
	C4 c = c4(p[0], p[1], p[2], 1.f);
	float h = 0.f, s = 0.f, v = 0.f;
	rgbToHsv(c, h, s, v);
	s *= sat_hue[2 * (size_t)i];
	h += sat_hue[2 * (size_t)i + 1];
	if(h < 0.f) h += 6.f;
	else if(h > 6.f) h -= 6.f;
	hsvToRgb(c, h, s, v);
	o[3 * (size_t)i] = c.r; o[3 * (size_t)i + 1] = c.g; o[3 * (size_t)i + 2] = c.b;
}
YD void texCubic(const float *in, float *o, int i)
{
	const float *p = in + 17 * (size_t)i;
	const C4 r = cubicInterp(ld4(p), ld4(p + 4), ld4(p + 8), ld4(p + 12), p[16]);
	o[4 * (size_t)i] = r.r; o[4 * (size_t)i + 1] = r.g; o[4 * (size_t)i + 2] = r.b; o[4 * (size_t)i + 3] = r.a;
}
// blendRgb on (tex, out) colours and blendValue on their first components
YD void texBlend(int mode, const float *tex, const float *out, const float *fact, const float *facg, float *o_rgb, float *o_val, int i)
{
	const float *t = tex + 3 * (size_t)i, *u = out + 3 * (size_t)i;
	const C3 r = blendRgb(C3{t[0], t[1], t[2]}, C3{u[0], u[1], u[2]}, fact[i], facg[i], mode);
	o_rgb[3 * (size_t)i] = r.r; o_rgb[3 * (size_t)i + 1] = r.g; o_rgb[3 * (size_t)i + 2] = r.b;
	o_val[i] = blendValue(t[0], u[0], fact[i], facg[i], mode);
}
__global__ void k_tex_pow(const float *ab, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i < n) o[i] = texPow(ab, i);
}
__global__ void k_tex_color_space(int cs, float gamma, const float *rgb, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i < n) texColorSpace(cs, gamma, rgb, o, i);
}
__global__ void k_tex_hsv(const float *rgb, const float *sat_hue, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i < n) texHsv(rgb, sat_hue, o, i);
}
__global__ void k_tex_cubic(const float *in, float *o, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i < n) texCubic(in, o, i);
}
__global__ void k_tex_blend(int mode, const float *tex, const float *out, const float *fact, const float *facg, float *o_rgb,
                            float *o_val, int n)
{
	const int i = blockIdx.x * kBlock + threadIdx.x;
	if(i < n) texBlend(mode, tex, out, fact, facg, o_rgb, o_val, i);
}
}

// Every wrapper returns the first non-zero hipError_t (0: all of allocate, copy in, launch, synchronise, copy out and
// free succeeded).
extern "C" {
int dd_round(const double *hi, const double *lo, int n, double *r_hi, double *r_lo, float *r24)
{
	Call k;
	const double *dh = k.in(hi, n), *dl = k.in(lo, n);
	double *oh = k.out<double>(n), *ol = k.out<double>(n);
	float *of = k.out<float>(n);
	if(k.ready(n)) { k_round<<<k.grid(n), kBlock>>>(dh, dl, n, oh, ol, of); k.ran(); }
	k.back(r_hi, oh, n); k.back(r_lo, ol, n); k.back(r24, of, n);
	return k.done();
}
int dd_x87mul(int c, const float *x, float *disp, float *exact, int n)
{
	Call k;
	const float *dx = k.in(x, n);
	float *dd = k.out<float>(n), *de = k.out<float>(n);
	if(k.ready(n)) { k_x87mul<<<k.grid(n), kBlock>>>(c, dx, dd, de, n); k.ran(); }
	k.back(disp, dd, n); k.back(exact, de, n);
	return k.done();
}
int dd_x87mul2(int c, const float *x, const float *y, float *disp, float *exact, int n)
{
	Call k;
	const float *dx = k.in(x, n), *dy = k.in(y, n);
	float *dd = k.out<float>(n), *de = k.out<float>(n);
	if(k.ready(n)) { k_x87mul2<<<k.grid(n), kBlock>>>(c, dx, dy, dd, de, n); k.ran(); }
	k.back(disp, dd, n); k.back(exact, de, n);
	return k.done();
}
int dd_x87mul3(int c, const float *x, const float *y, const float *z, float *disp, float *exact, int n)
{
	Call k;
	const float *dx = k.in(x, n), *dy = k.in(y, n), *dz = k.in(z, n);
	float *dd = k.out<float>(n), *de = k.out<float>(n);
	if(k.ready(n)) { k_x87mul3<<<k.grid(n), kBlock>>>(c, dx, dy, dz, dd, de, n); k.ran(); }
	k.back(disp, dd, n); k.back(exact, de, n);
	return k.done();
}
int dd_x87muldiv(int c, const float *a, const float *b, float *disp, float *exact, int n)
{
	Call k;
	const float *da = k.in(a, n), *db = k.in(b, n);
	float *dd = k.out<float>(n), *de = k.out<float>(n);
	if(k.ready(n)) { k_x87muldiv<<<k.grid(n), kBlock>>>(c, da, db, dd, de, n); k.ran(); }
	k.back(disp, dd, n); k.back(exact, de, n);
	return k.done();
}
int dd_x87recip(int c, const float *a, float *disp, float *exact, int n)
{
	Call k;
	const float *da = k.in(a, n);
	float *dd = k.out<float>(n), *de = k.out<float>(n);
	if(k.ready(n)) { k_x87recip<<<k.grid(n), kBlock>>>(c, da, dd, de, n); k.ran(); }
	k.back(disp, dd, n); k.back(exact, de, n);
	return k.done();
}
int dd_x87one_minus(int c, const float *x, float *disp, int n)
{
	Call k;
	const float *dx = k.in(x, n);
	float *dd = k.out<float>(n);
	if(k.ready(n)) { k_x87one_minus<<<k.grid(n), kBlock>>>(c, dx, dd, n); k.ran(); }
	k.back(disp, dd, n);
	return k.done();
}
// out: 5 arrays in the order atan2f(y, x), acosf(y), asinf(y), atanf(y), math::asin(y)
int dd_libm_all(const float *y, const float *x, int n, float *const *out)
{
	Call k;
	const float *dy = k.in(y, n), *dx = k.in(x, n);
	float *d[5];
	for(float *&p : d) p = k.out<float>(n);
	if(k.ready(n)) { k_libm<<<k.grid(n), kBlock>>>(dy, dx, n, d[0], d[1], d[2], d[3], d[4]); k.ran(); }
	for(int j = 0; j < 5; ++j) k.back(out[j], d[j], n);
	return k.done();
}
int dd_sincos(const float *x, float *o_sin, float *o_cos, int n)
{
	Call k;
	const float *dx = k.in(x, n);
	float *ds = k.out<float>(n), *dc = k.out<float>(n);
	if(k.ready(n)) { k_sincos<<<k.grid(n), kBlock>>>(dx, ds, dc, n); k.ran(); }
	k.back(o_sin, ds, n); k.back(o_cos, dc, n);
	return k.done();
}
int dd_hemi(const float *p, const float *s, float *o, int n)
{
	Call k;
	const float *dp = k.in(p, 9 * (size_t)n), *ds = k.in(s, 2 * (size_t)n);
	float *d = k.out<float>(3 * (size_t)n);
	if(k.ready(n)) { k_hemi<<<k.grid(n), kBlock>>>(dp, ds, d, n); k.ran(); }
	k.back(o, d, 3 * (size_t)n);
	return k.done();
}
int dd_coords(const float *in, float *o, int n)
{
	Call k;
	const float *di = k.in(in, 3 * (size_t)n);
	float *d = k.out<float>(6 * (size_t)n);
	if(k.ready(n)) { k_coords<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(o, d, 6 * (size_t)n);
	return k.done();
}
int dd_normalize(const float *in, float *o, int n)
{
	Call k;
	const float *di = k.in(in, 3 * (size_t)n);
	float *d = k.out<float>(3 * (size_t)n);
	if(k.ready(n)) { k_normalize<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(o, d, 3 * (size_t)n);
	return k.done();
}
int dd_ri(int which, const uint32_t *b, const uint32_t *r, float *o, int n)
{
	Call k;
	const uint32_t *db = k.in(b, n), *dr = k.in(r, n);
	float *d = k.out<float>(n);
	if(k.ready(n)) { k_ri<<<k.grid(n), kBlock>>>(which, db, dr, d, n); k.ran(); }
	k.back(o, d, n);
	return k.done();
}
int dd_fnv(const uint32_t *in, uint32_t *o, int n)
{
	Call k;
	const uint32_t *di = k.in(in, n);
	uint32_t *d = k.out<uint32_t>(n);
	if(k.ready(n)) { k_fnv<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(o, d, n);
	return k.done();
}
int dd_bitrev(const uint32_t *in, uint32_t *o, int n)
{
	Call k;
	const uint32_t *di = k.in(in, n);
	uint32_t *d = k.out<uint32_t>(n);
	if(k.ready(n)) { k_bitrev<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(o, d, n);
	return k.done();
}
int dd_udiv(uint32_t dv, const uint32_t *in, uint32_t *o, int n)
{
	Call k;
	const uint32_t *di = k.in(in, n);
	uint32_t *d = k.out<uint32_t>(n);
	if(k.ready(n)) { k_udiv<<<k.grid(n), kBlock>>>(dv, di, d, n); k.ran(); }
	k.back(o, d, n);
	return k.done();
}
// perm: the `base` entries of the dimension's Faure permutation
int dd_lds(const uint8_t *perm, uint32_t base, double f, const uint32_t *idx, double *o, int n)
{
	Call k;
	const uint8_t *dp = k.in(perm, base);
	const uint32_t *di = k.in(idx, n);
	double *d = k.out<double>(n);
	if(k.ready(n)) { k_lds<<<k.grid(n), kBlock>>>(dp, base, f, di, d, n); k.ran(); }
	k.back(o, d, n);
	return k.done();
}
int dd_mwc(const uint32_t *seed, int steps, double *o, int n)
{
	Call k;
	const uint32_t *ds = k.in(seed, n);
	double *d = k.out<double>((size_t)n * steps);
	if(k.ready(n)) { k_mwc<<<k.grid(n), kBlock>>>(ds, steps, d, n); k.ran(); }
	k.back(o, d, (size_t)n * steps);
	return k.done();
}
int dd_halton(uint32_t base, const uint32_t *start, int n, int kk, float *first, float *next, float *inc)
{
	Call k;
	const uint32_t *ds = k.in(start, n);
	float *df = k.out<float>(n), *dn = k.out<float>((size_t)n * kk), *di = k.in(inc, (size_t)n * kk);
	if(k.ready(n)) { k_halton<<<k.grid(n), kBlock>>>(base, ds, n, kk, df, dn, di); k.ran(); }
	k.back(first, df, n); k.back(next, dn, (size_t)n * kk); k.back(inc, di, (size_t)n * kk);
	return k.done();
}

// texeval.h: `dev` from the kernel, `host` from this translation unit's host pass
int dd_tex_pow(const float *ab, float *dev, float *host, int n)
{
	for(int i = 0; i < n; ++i) host[i] = texPow(ab, i);
	Call k;
	const float *di = k.in(ab, 2 * (size_t)n);
	float *d = k.out<float>(n);
	if(k.ready(n)) { k_tex_pow<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(dev, d, n);
	return k.done();
}
int dd_tex_color_space(int cs, float gamma, const float *rgb, float *dev, float *host, int n)
{
	for(int i = 0; i < n; ++i) texColorSpace(cs, gamma, rgb, host, i);
	Call k;
	const float *di = k.in(rgb, 3 * (size_t)n);
	float *d = k.out<float>(3 * (size_t)n);
	if(k.ready(n)) { k_tex_color_space<<<k.grid(n), kBlock>>>(cs, gamma, di, d, n); k.ran(); }
	k.back(dev, d, 3 * (size_t)n);
	return k.done();
}
int dd_tex_hsv(const float *rgb, const float *sat_hue, float *dev, float *host, int n)
{
	for(int i = 0; i < n; ++i) texHsv(rgb, sat_hue, host, i);
	Call k;
	const float *di = k.in(rgb, 3 * (size_t)n), *ds = k.in(sat_hue, 2 * (size_t)n);
	float *d = k.out<float>(3 * (size_t)n);
	if(k.ready(n)) { k_tex_hsv<<<k.grid(n), kBlock>>>(di, ds, d, n); k.ran(); }
	k.back(dev, d, 3 * (size_t)n);
	return k.done();
}
int dd_tex_cubic(const float *in, float *dev, float *host, int n)
{
	for(int i = 0; i < n; ++i) texCubic(in, host, i);
	Call k;
	const float *di = k.in(in, 17 * (size_t)n);
	float *d = k.out<float>(4 * (size_t)n);
	if(k.ready(n)) { k_tex_cubic<<<k.grid(n), kBlock>>>(di, d, n); k.ran(); }
	k.back(dev, d, 4 * (size_t)n);
	return k.done();
}
int dd_tex_blend(int mode, const float *tex, const float *out, const float *fact, const float *facg, float *dev_rgb, float *dev_val,
                 float *host_rgb, float *host_val, int n)
{
	for(int i = 0; i < n; ++i) texBlend(mode, tex, out, fact, facg, host_rgb, host_val, i);
	Call k;
	const float *dt = k.in(tex, 3 * (size_t)n), *du = k.in(out, 3 * (size_t)n), *df = k.in(fact, n), *dg = k.in(facg, n);
	float *dr = k.out<float>(3 * (size_t)n), *dv = k.out<float>(n);
	if(k.ready(n)) { k_tex_blend<<<k.grid(n), kBlock>>>(mode, dt, du, df, dg, dr, dv, n); k.ran(); }
	k.back(dev_rgb, dr, 3 * (size_t)n); k.back(dev_val, dv, n);
	return k.done();
}
}
