// Host build of the device numerics (libyafaray_amd/csrc/devmath.h) with extern "C" wrappers, so
// tests/test_devmath.py can pin the exact code the kernels run against the reference's golden
// vectors (tests/golden/prims.npz).  Compiled with g++ -ffp-contract=off at test time.
#include "../libyafaray_amd/csrc/devmath.h"
using namespace yafamd;
extern "C" {
void dm_ri(int which, const uint32_t *b, const uint32_t *r, float *o, int n)
{
	for(int i = 0; i < n; ++i) o[i] = which == 0 ? riVdC(b[i], r[i]) : which == 1 ? riS(b[i], r[i]) : riLp(b[i], r[i]);
}
int dm_udiv_check(uint32_t d, const uint32_t *n, int cnt)
{
	const UDiv q = udivMake(d);
	for(int i = 0; i < cnt; ++i) if(udiv(n[i], q) != n[i] / d) return i;
	return -1;
}
void dm_fnv(const uint32_t *in, uint32_t *o, int n) { for(int i = 0; i < n; ++i) o[i] = fnv32(in[i]); }
void dm_lds(const uint8_t *perm, uint32_t base, double f, const uint32_t *idx, double *o, int n)
{
	const UDiv dv = udivMake(base);
	for(int i = 0; i < n; ++i) o[i] = lowDiscrepancy(perm, base, dv, f, idx[i]);
}
void dm_halton_first(uint32_t base, const uint32_t *start, float *o, int n)
{
	for(int i = 0; i < n; ++i) o[i] = haltonFirst(base, 1.0 / (double)base, start[i]);
}
void dm_sin(const float *x, float *o, int n) { for(int i = 0; i < n; ++i) o[i] = fsin(x[i]); }
void dm_cos(const float *x, float *o, int n) { for(int i = 0; i < n; ++i) o[i] = fcos(x[i]); }
void dm_hemi(const float *p, const float *s, float *o, int n)
{
	for(int i = 0; i < n; ++i)
	{
		const float *q = p + 9 * i;
		const V3 r = cosHemisphere(v3(q[0], q[1], q[2]), v3(q[3], q[4], q[5]), v3(q[6], q[7], q[8]), s[2 * i], s[2 * i + 1]);
		o[3 * i] = r.x; o[3 * i + 1] = r.y; o[3 * i + 2] = r.z;
	}
}
void dm_coords(const float *in, float *o, int n)
{
	for(int i = 0; i < n; ++i)
	{
		V3 u, v;
		coordsSystem(v3(in[3 * i], in[3 * i + 1], in[3 * i + 2]), u, v);
		o[6 * i] = u.x; o[6 * i + 1] = u.y; o[6 * i + 2] = u.z; o[6 * i + 3] = v.x; o[6 * i + 4] = v.y; o[6 * i + 5] = v.z;
	}
}
void dm_normalize(const float *in, float *o, int n)
{
	for(int i = 0; i < n; ++i)
	{
		const V3 r = normalize(v3(in[3 * i], in[3 * i + 1], in[3 * i + 2]));
		o[3 * i] = r.x; o[3 * i + 1] = r.y; o[3 * i + 2] = r.z;
	}
}
void dm_mwc(uint32_t seed, int steps, double *o)
{
	Mwc m{30903u, seed};
	for(int i = 0; i < steps; ++i) o[i] = m.next();
}
// libm restatements (devmath.h libmAtan2f / libmAcosf) next to the host's own libm on the same inputs;
// the sphere mapping's long double expression next to real x87 long double
void dm_libm(const float *y, const float *x, int n, float *dev_atan2, float *libm_atan2, float *dev_acos, float *libm_acos)
{
	for(int i = 0; i < n; ++i)
	{
		dev_atan2[i] = libmAtan2f(y[i], x[i]);
		libm_atan2[i] = ::atan2f(y[i], x[i]);
		dev_acos[i] = libmAcosf(y[i]);
		libm_acos[i] = ::acosf(y[i]);
	}
}
void dm_sphere_v(const float *a, int n, float *dev, float *ref)
{
	const long double div_1_by_pi = 0.31830988618379067153776752674503L;   // include/math/math.h
	for(int i = 0; i < n; ++i)
	{
		dev[i] = x87oneMinus2Mul(kDiv1ByPi, a[i]);
		ref[i] = static_cast<float>(1.f - 2.f * (a[i] * div_1_by_pi));
	}
}
}

// ---------------------------------------------------------------------------------------------
// The entry points below have twins of the same shape in tests/devmath_dev.hip (dd_*), which run the
// same functions on the device; tests/test_devmath_gpu.py compares the two bit for bit.
// ---------------------------------------------------------------------------------------------
namespace
{
// the long double constants by index, as (hi, lo) pairs and as the reference writes them (include/math/math.h)
const X87Const kConsts[7] = {kPi, kDivPiBy2, kDiv1ByPi, kMultPiBy2, kDiv1By2Pi, kDiv4ByPi, kDiv4BySquaredPi};
const long double kConstsLd[7] = {3.1415926535897932384626433832795L, 1.5707963267948966192313216916398L,
                                  0.31830988618379067153776752674503L, 6.283185307179586476925286766559L,
                                  0.15915494309189533576888376337251L, 1.2732395447351626861510701069801L,
                                  0.40528473456935108577551785283891L};
// the double a dispatcher hands to safeToRound
enum { SCAN_MUL = 0, SCAN_MUL2_ABS, SCAN_MUL2, SCAN_MUL3, SCAN_MULDIV, SCAN_RECIP };
double dispatchApprox(int which, const X87Const &c, float x, float y, float z)
{
	switch(which)
	{
		case SCAN_MUL: return c.hi * (double)x;
		case SCAN_MUL2_ABS: return c.hi * (double)x * (double)fabsf(x);
		case SCAN_MUL2: return c.hi * (double)x * (double)y;
		case SCAN_MUL3: return c.hi * (double)x * (double)y * (double)z;
		case SCAN_MULDIV: return c.hi * (double)x / (double)y;
		default: return 1.0 / (c.hi * (double)x);
	}
}
}

extern "C" {
// Every positive float of one binade (biased exponent `expo`, all 2^23 significands) through the fast-path test
// of a dispatcher (which: SCAN_*, constant c, the other operands y and z): the inputs for which safeToRound is
// false, i.e. that take the exact (slow) branch.  Returns how many there are; the first `cap` are stored.
int dm_scan_binade(int which, int c, int expo, float y, float z, float *out, int cap)
{
	int found = 0;
	for(uint32_t m = 0; m < (1u << 23); ++m)
	{
		const float x = bitsf(((uint32_t)expo << 23) | m);
		float f;
		if(safeToRound(dispatchApprox(which, kConsts[c], x, y, z), f)) continue;
		if(found < cap) out[found] = x;
		++found;
	}
	return found;
}
// The two rounding steps every exact path ends with, on a caller-made double-double (hi, lo): r = round64(v) and
// round24(r), with real x87 arithmetic beside them: (long double)hi + lo is the exact sum rounded once to a 64-bit
// significand (ok64: r's two parts add up to it exactly), and its float cast is the second rounding (ref24).
void dm_round(const double *hi, const double *lo, int n, double *r_hi, double *r_lo, float *r24, int32_t *ok64, float *ref24)
{
	for(int i = 0; i < n; ++i)
	{
		const DD r = round64(DD{hi[i], lo[i]});
		r_hi[i] = r.hi;
		r_lo[i] = r.lo;
		r24[i] = round24(r);
		const long double s = (long double)hi[i] + (long double)lo[i];
		ok64[i] = (long double)r.hi + (long double)r.lo == s;
		ref24[i] = (float)s;
	}
}
// the dispatchers, their exact paths on every input, and the reference expression in real long double
void dm_x87mul(int c, const float *x, float *disp, float *exact, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87mul(kConsts[c], x[i]);
		exact[i] = x87mulExact(kConsts[c].hi, kConsts[c].lo, x[i]);
		ld[i] = (float)(kConstsLd[c] * x[i]);
	}
}
void dm_x87mul2(int c, const float *x, const float *y, float *disp, float *exact, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87mul2(kConsts[c], x[i], y[i]);
		exact[i] = x87mul2Exact(kConsts[c].hi, kConsts[c].lo, x[i], y[i]);
		ld[i] = (float)(kConstsLd[c] * x[i] * y[i]);
	}
}
void dm_x87mul3(int c, const float *x, const float *y, const float *z, float *disp, float *exact, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87mul3(kConsts[c], x[i], y[i], z[i]);
		exact[i] = x87mul3Exact(kConsts[c].hi, kConsts[c].lo, x[i], y[i], z[i]);
		ld[i] = (float)(kConstsLd[c] * x[i] * y[i] * z[i]);
	}
}
void dm_x87muldiv(int c, const float *a, const float *b, float *disp, float *exact, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87mulDiv(kConsts[c], a[i], b[i]);
		exact[i] = x87mulDivExact(kConsts[c].hi, kConsts[c].lo, a[i], b[i]);
		ld[i] = (float)(a[i] * kConstsLd[c] / b[i]);
	}
}
void dm_x87recip(int c, const float *a, float *disp, float *exact, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87recipMul(kConsts[c], a[i]);
		exact[i] = x87recipMulExact(kConsts[c].hi, kConsts[c].lo, a[i]);
		ld[i] = (float)(1.f / (a[i] * kConstsLd[c]));
	}
}
void dm_x87one_minus(int c, const float *x, float *disp, float *ld, int n)
{
	for(int i = 0; i < n; ++i)
	{
		disp[i] = x87oneMinus2Mul(kConsts[c], x[i]);
		ld[i] = (float)(1.f - 2.f * (x[i] * kConstsLd[c]));
	}
}
// every libm restatement with the host's libm beside it (out: 5 x 2 arrays, restatement then libm, in the order
// atan2f(y, x), acosf(y), asinf(y), atanf(y), math::asin(y))
void dm_libm_all(const float *y, const float *x, int n, float *const *dev, float *const *ref)
{
	for(int i = 0; i < n; ++i)
	{
		dev[0][i] = libmAtan2f(y[i], x[i]);
		ref[0][i] = ::atan2f(y[i], x[i]);
		dev[1][i] = libmAcosf(y[i]);
		ref[1][i] = ::acosf(y[i]);
		dev[2][i] = libmAsinf(y[i]);
		ref[2][i] = ::asinf(y[i]);
		dev[3][i] = libmAtanf(y[i]);
		ref[3][i] = ::atanf(y[i]);
		dev[4][i] = mathAsin(y[i]);
		// math.h:260-266
		ref[4][i] = y[i] <= -1.f ? -(float)kConstsLd[1] : y[i] >= 1.f ? (float)kConstsLd[1] : ::asinf(y[i]);
	}
}
// Halton(base, start): getNext() of a fresh generator, the value after each of k getNext() calls by haltonNext, and
// the same k values from the running generator (bases 2, 3 and 5; `inc` untouched for another base)
void dm_halton(uint32_t base, const uint32_t *start, int n, int k, float *first, float *next, float *inc)
{
	for(int i = 0; i < n; ++i)
	{
		first[i] = haltonFirst(base, 1.0 / (double)base, start[i]);
		for(int j = 0; j < k; ++j) next[(size_t)i * k + j] = haltonNext(base, start[i], j + 1);
		float *o = inc + (size_t)i * k;
		if(base == 2) { HaltonInc<2> h; h.start(start[i]); for(int j = 0; j < k; ++j) o[j] = h.next(); }
		else if(base == 3) { HaltonInc<3> h; h.start(start[i]); for(int j = 0; j < k; ++j) o[j] = h.next(); }
		else if(base == 5) { HaltonInc<5> h; h.start(start[i]); for(int j = 0; j < k; ++j) o[j] = h.next(); }
	}
}
void dm_bitrev(const uint32_t *in, uint32_t *o, int n) { for(int i = 0; i < n; ++i) o[i] = bitReverse32(in[i]); }
void dm_udiv(uint32_t d, const uint32_t *in, uint32_t *o, int n)
{
	const UDiv q = udivMake(d);
	for(int i = 0; i < n; ++i) o[i] = udiv(in[i], q);
}
}
