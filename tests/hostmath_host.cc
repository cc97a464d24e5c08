// The product's host numerics of the film (libyafaray_amd/csrc/hostmath.h) with extern "C" wrappers, so
// tests/filmlib.py can pin the exact code host.cc runs: the four filter functions against the reference's
// golden vectors (tests/golden/prims.npz, prims_filters.npz) and the film set-up (filter half-width, table
// scale, footprint reach, the 16 x 16 table) against the oracle's.  Compiled with g++ -ffp-contract=off at
// test time, like devmath_host.cc.
#include "../libyafaray_amd/csrc/hostmath.h"
using namespace yafamd;
extern "C" {
// which: hm::FilmFilter (0 box, 1 gauss, 2 mitchell, 3 lanczos); dxdy: 2 floats per element
void hmh_filter(int which, const float *dxdy, float *o, int n)
{
	float (*ff)(float, float) = which == hm::FILM_GAUSS ? hm::filterGauss : which == hm::FILM_MITCHELL ? hm::filterMitchell
	                            : which == hm::FILM_LANCZOS ? hm::filterLanczos : hm::filterBox;
	for(int i = 0; i < n; ++i) o[i] = ff(dxdy[2 * i], dxdy[2 * i + 1]);
}
// the set-up host.cc hands to the film kernels: reach = (reach_fwd, reach_back)
void hmh_film_setup(int filter, float pixelwidth, float *table16x16, float *filterw, float *table_scale, int *reach)
{
	const hm::FilmSetup F = hm::filmSetup(filter, pixelwidth);
	std::memcpy(table16x16, F.table, sizeof(F.table));
	*filterw = F.filterw;
	*table_scale = F.table_scale;
	reach[0] = F.reach_fwd;
	reach[1] = F.reach_back;
}
}
