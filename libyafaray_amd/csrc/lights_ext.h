// Spot, directional, sun and sphere lights (src/light/light_spot.cc, light_directional.cc, light_sun.cc,
// light_sphere.cc): their illuminate / illumSample / intersect / emitPhoton bodies with the reference's
// float expressions.  Included by kernels.hip after devmath.h, rcpExact, shirleyDisk (camera.h) and lv (sphereDir is
// declared below); only the XL instantiations (DevScene::has_ext_light) call into it.
//
// DevLight fields per type (host.cc Scene::createLight, initBoundLight):
//   spot        pos = position, fnormal = ndir (towards the light), to_x = dir, du / dv,
//               c2 = (cos_start, cos_end, icos_diff, -), c3 = (interv_1, interv_2, ipdf of interval 1, -)
//   directional pos = position, fnormal = direction, du / dv, c2 = (radius, world radius, infinite, ipdf)
//   sun         fnormal = direction, du / dv (of the un-normalised direction, light_sun.cc:36),
//               c2 = (cos_angle, invpdf, pdf, e_pdf), c3 = (world centre, world radius), c4 = col_pdf * e_pdf,
//               color = col_pdf, to_x = color * power (totalEnergy)
//   sphere      pos = centre, c2 = (radius, radius^2, radius^2 * 1.000003815, -), area
#pragma once

// (kernels.hip includes this inside namespace yafamd)
__device__ __forceinline__ V3 sphereDir(float s_1, float s_2);

// sample.h:80-86
__device__ __forceinline__ V3 sampleCone(V3 d, V3 u, V3 v, float max_cos_ang, float s_1, float s_2)
{
	const float cos_ang = 1.f - (1.f - max_cos_ang) * s_2;
	const float sin_ang = sqrtf(1.f - cos_ang * cos_ang);
	const float t_1 = x87mul(kMultPiBy2, s_1);
	return (u * fcos(t_1) + v * fsin(t_1)) * sin_ang + d * cos_ang;
}

// sample.h:92-100 (the middle term is a Vec3 of three equal components)
__device__ __forceinline__ void minRot(V3 d, V3 u, V3 d_2, V3 &u_2, V3 &v_2)
{
	const float cos_alpha = dot(d, d_2);
	const float sin_alpha = sqrtf(1.f - cos_alpha * cos_alpha);
	const V3 v = cross(d, d_2);
	const float mid = (1.f - cos_alpha) * dot(v, u);
	u_2 = cos_alpha * u + v3(mid, mid, mid) + sin_alpha * cross(v, u);
	v_2 = cross(d_2, u_2);
}

__device__ __forceinline__ bool lightIsDirac(const DevLight &L) { return L.type == LIGHT_SPOT || L.type == LIGHT_DIRECTIONAL; }

// the smoothstep of the spot's blend zone (light_spot.cc:94-95)
__device__ __forceinline__ float spotFalloff(const DevLight &L, float cosa)
{
	float v = (cosa - L.c2[1]) * L.c2[2];
	v = v * v * (3.f - 2.f * v);
	return v;
}

// SpotLight::illuminate (light_spot.cc:73-102) / DirectionalLight::illuminate (light_directional.cc:58-79):
// the light colour at p, the direction to the light and the light ray's tmax (-1: no end)
__device__ __forceinline__ bool diracIlluminate(const DevLight &L, V3 p, C3 &col, V3 &ldir, float &tmax)
{
	const C3 color = C3{L.color[0], L.color[1], L.color[2]};
	if(L.type == LIGHT_SPOT)
	{
		ldir = lv(L.pos) - p;
		const float dist_sqr = dot(ldir, ldir);
		const float dist = sqrtf(dist_sqr);
		if((double)dist == 0.0) return false;
		const float idist_sqr = rcpExact(dist_sqr);
		ldir = ldir * rcpExact(dist);
		const float cosa = dot(lv(L.fnormal), ldir);
		if(cosa < L.c2[1]) return false;
		if(cosa >= L.c2[0]) col = color * idist_sqr;
		else col = color * spotFalloff(L, cosa) * idist_sqr;
		tmax = dist;
		return true;
	}
	const V3 direction = lv(L.fnormal);
	if(L.c2[2] == 0.f)
	{
		const V3 vec = lv(L.pos) - p;
		const float dist = length(cross(direction, vec));
		if(dist > L.c2[0]) return false;
		tmax = dot(vec, direction);
		if((double)tmax <= 0.0) return false;
	}
	else tmax = -1.f;
	ldir = direction;
	col = color;
	return true;
}

// SphereLight::sphereIntersect (light_sphere.cc:55-67): the double promotions of the discriminant and the roots
__device__ __forceinline__ bool sphereLightIntersect(V3 from, V3 dir, V3 c, float r_2, float &d_1)
{
	const V3 vf = from - c;
	const float ea = dot(dir, dir);
	const float eb = dot(2.f * vf, dir);
	const float ec = dot(vf, vf) - r_2;
	float osc = (float)((double)(eb * eb) - 4.0 * (double)ea * (double)ec);
	if(osc < 0)
	{
		d_1 = sqrtf(ec / ea);
		return false;
	}
	osc = sqrtf(osc);
	d_1 = (float)((double)(-eb - osc) / (2.0 * (double)ea));
	return true;
}

// SunLight::illumSample (light_sun.cc:54-67) / SphereLight::illumSample (light_sphere.cc:69-99): direction,
// the light ray's tmax (-1: no end) and the pdf; the colour is L.color for both
__device__ __forceinline__ bool extIllumSample(const DevLight &L, V3 p, float s_1, float s_2, V3 &ldir, float &tmax, float &pdf)
{
	if(L.type == LIGHT_SUN)
	{
		ldir = sampleCone(lv(L.fnormal), lv(L.du), lv(L.dv), L.c2[0], s_1, s_2);
		tmax = -1.f;
		pdf = L.c2[2];
		return true;
	}
	V3 cdir = lv(L.pos) - p;
	const float dist_sqr = lengthSqr(cdir);
	if(dist_sqr <= L.c2[1]) return false;   // light on the outside only
	const float dist = sqrtf(dist_sqr);
	const float idist_sqr = rcpExact(dist_sqr);
	const float cos_alpha = sqrtf(1.f - L.c2[1] * idist_sqr);
	cdir = cdir * rcpExact(dist);
	V3 cu, cv;
	coordsSystem(cdir, cu, cv);
	ldir = sampleCone(cdir, cu, cv, cos_alpha, s_1, s_2);
	float d_1;
	if(!sphereLightIntersect(p, ldir, lv(L.pos), L.c2[2], d_1)) return false;
	tmax = d_1;
	pdf = rcpExact(2.f * (1.f - cos_alpha));
	return true;
}

// SunLight::intersect (light_sun.cc:69-77): the material-sampled direction falls into the sun's cone
__device__ __forceinline__ bool sunIntersect(const DevLight &L, V3 dir, float &t, float &ipdf)
{
	const float cosine = dot(dir, lv(L.fnormal));
	if(cosine < L.c2[0]) return false;
	t = -1.f;
	ipdf = L.c2[1];
	return true;
}

// Pdf1D::sample (sample_pdf1d.h:96-121) over the spot's 65-entry smoothstep table: tab = 65 function values,
// then the 65 cdf values, then (integral, 1 / integral, 1 / 65)
__device__ __forceinline__ float spotPdfSample(const float *tab, float u, float &pdf)
{
	const float *func = tab, *cdf = tab + 65;
	const float inv_integral = tab[131];
	if(u <= 0.f)
	{
		pdf = func[0] * inv_integral;
		return 0.f;
	}
	if(u >= 1.f)
	{
		pdf = func[64] * inv_integral;
		return 64.f + 1.f;
	}
	int lo = 0, hi = 65;   // std::lower_bound
	while(lo < hi)
	{
		const int mid = (lo + hi) >> 1;
		if(cdf[mid] < u) lo = mid + 1;
		else hi = mid;
	}
	const int index = lo < 65 ? lo : 64;   // (cdf[64] is 1: u < 1 never passes it)
	pdf = func[index] * inv_integral;
	const float delta = index > 0 ? (u - cdf[index - 1]) / (cdf[index] - cdf[index - 1]) : u / cdf[index];
	return (float)index + delta;
}

// emitPhoton of the four types (light_spot.cc:145-166, light_directional.cc:89-99, light_sun.cc:79-94,
// light_sphere.cc:136-144): origin, direction, ipdf and the returned colour
__device__ __forceinline__ C3 extEmitPhoton(const DevScene &S, const DevLight &L, float s_1, float s_2, float s_3, float s_4, V3 &o, V3 &d, float &ipdf)
{
	const C3 color = C3{L.color[0], L.color[1], L.color[2]};
	if(L.type == LIGHT_SPOT)
	{
		o = lv(L.pos);
		const V3 dir = lv(L.to_x), du = lv(L.du), dv = lv(L.dv);
		const float cos_start = L.c2[0], cos_end = L.c2[1];
		if(s_3 <= L.c3[0])
		{
			d = sampleCone(dir, du, dv, cos_start, s_1, s_2);
			ipdf = L.c3[2];
			return color;
		}
		float spdf;
		const float sm_2 = spotPdfSample(S.spot_pdf, s_2, spdf) * S.spot_pdf[132];
		ipdf = x87mulDiv(kMultPiBy2, cos_start - cos_end, L.c3[1] * spdf);
		const double cos_ang = (double)cos_end + (double)(cos_start - cos_end) * (double)sm_2;
		const double sin_ang = (double)sqrtf((float)(1.0 - cos_ang * cos_ang));
		const float t_1 = x87mul(kMultPiBy2, s_1);
		d = (du * fcos(t_1) + dv * fsin(t_1)) * (float)sin_ang + dir * (float)cos_ang;
		return color * spdf * S.spot_pdf[130];
	}
	if(L.type == LIGHT_DIRECTIONAL)
	{
		const V3 direction = lv(L.fnormal);
		d = -direction;
		float u, v;
		shirleyDisk(s_1, s_2, u, v);
		o = lv(L.pos) + L.c2[0] * (u * lv(L.du) + v * lv(L.dv));
		if(L.c2[2] != 0.f) o = o + direction * L.c2[1];
		ipdf = L.c2[3];
		return color;
	}
	if(L.type == LIGHT_SUN)
	{
		float u, v;
		shirleyDisk(s_3, s_4, u, v);
		const V3 direction = lv(L.fnormal), du = lv(L.du);
		const V3 ldir = sampleCone(direction, du, lv(L.dv), L.c2[0], s_3, s_4);
		V3 du_2, dv_2;
		minRot(direction, du, ldir, du_2, dv_2);
		ipdf = L.c2[1];
		o = lv(L.c3) + L.c3[3] * (u * du_2 + v * dv_2 + ldir);
		d = -ldir;
		return C3{L.c4[0], L.c4[1], L.c4[2]};
	}
	const V3 sdir = sphereDir(s_3, s_4);
	o = lv(L.pos) + L.c2[0] * sdir;
	V3 cu, cv;
	coordsSystem(sdir, cu, cv);
	d = cosHemisphere(sdir, cu, cv, s_1, s_2);
	ipdf = L.area;
	return color;
}
