"""Renders with k_trace's deferred leaf tests (YAFARAY_AMD_TRACE_DEFER=1) against the interleaved loop (=0):
a Cornell render at 64 x 48 x 4 spp, depth 4, must give the same film bits, weights, ray and sample counts with
Russian roulette on and off, under the serial and the overlapped schedule, with 2 / 5 / the default number of
queue segments (YAFARAY_AMD_SHADE_GRID), and twice on one Interface.  The traversal's own counters (node visits,
triangle tests) belong to the loop that ran: with DEFER=1 they are equal between the serial and the overlapped
schedule (a ray's visits and tests do not depend on the rays it shares a wave with) and differ from DEFER=0's on
this scene, which shows that the switch selects another loop.  Renders that are not eligible (transparent
shadows, a scene in global memory) launch the same kernels under both settings: equal results and equal
counters."""
import numpy as np
import pytest

from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

ENV = ("YAFARAY_AMD_TRACE_DEFER", "YAFARAY_AMD_TRACE_DEFER_CAP", "YAFARAY_AMD_TRACE_DEFER_IT0", "YAFARAY_AMD_OVERLAP",
       "YAFARAY_AMD_OVERLAP_SHADOW", "YAFARAY_AMD_SHADE_GRID", "YAFARAY_AMD_SCENE_LDS")
RESULT = ("closest_rays", "shadow_rays", "samples")
TRAVERSAL = ("node_visits", "tri_tests")


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render(product, monkeypatch, spec, defer, overlap=None, shade_grid=None, env=None, trace_stats=False, renders=1):
    """[(rgba, weights, stats)] of `renders` renders on one Interface under the given settings."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("YAFARAY_AMD_TRACE_DEFER", str(defer))
    if overlap is not None:
        monkeypatch.setenv("YAFARAY_AMD_OVERLAP", str(overlap))
    if shade_grid is not None:
        monkeypatch.setenv("YAFARAY_AMD_SHADE_GRID", str(shade_grid))
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.L.yafaray_amd_setTraceStats(yi.h, 1 if trace_stats else 0)
    out = []
    for _ in range(renders):
        yi.render()
        rgba, w = yi.film()
        out.append((rgba.copy(), w.copy(), yi.stats()))
    yi.close()
    return out


def assert_same(a, b, counters=RESULT):
    (ra, wa, sa), (rb, wb, sb) = a, b
    assert np.array_equal(_bits(wa), _bits(wb)), f"{(wa != wb).sum()} weights differ"
    diff = _bits(ra) != _bits(rb)
    assert not diff.any(), f"{diff.sum()} film values differ, first at {np.argwhere(diff)[0]}"
    for k in counters:
        assert sa[k] == sb[k], (k, sa[k], sb[k])


def cornell(rr):
    return scenes.cornell(64, 48, spp=4, bounces=4, rr=rr)


@pytest.mark.parametrize("shade_grid", [2, 5, None])
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("rr", [False, True])
def test_deferred_render_equals_interleaved(product, monkeypatch, rr, overlap, shade_grid):
    spec = cornell(rr)
    a = render(product, monkeypatch, spec, 0, overlap, shade_grid)[0]
    b = render(product, monkeypatch, spec, 1, overlap, shade_grid)[0]
    assert_same(a, b)
    assert a[2]["closest_rays"] > 0 and a[2]["shadow_rays"] > 0
    # (the lists at their smallest capacity: lanes flush in the middle of their traversals)
    c = render(product, monkeypatch, spec, 1, overlap, shade_grid, env={"YAFARAY_AMD_TRACE_DEFER_CAP": "1"})[0]
    assert_same(a, c)


def test_deferred_two_renders_on_one_interface(product, monkeypatch):
    spec = cornell(True)
    a = render(product, monkeypatch, spec, 0)[0]
    b1, b2 = render(product, monkeypatch, spec, 1, renders=2)
    assert_same(a, b1)
    assert_same(a, b2)


@pytest.mark.parametrize("cap", [None, "1"])
def test_deferred_traversal_counters_do_not_depend_on_the_schedule(product, monkeypatch, cap):
    spec = cornell(True)
    env = {"YAFARAY_AMD_TRACE_DEFER_CAP": cap} if cap else None
    ser = render(product, monkeypatch, spec, 1, 0, env=env, trace_stats=True)[0]
    ovl = render(product, monkeypatch, spec, 1, 1, env=env, trace_stats=True)[0]
    assert_same(ser, ovl, counters=RESULT + TRAVERSAL)
    assert ser[2]["node_visits"] > 0 and ser[2]["tri_tests"] > 0
    two = render(product, monkeypatch, spec, 1, 1, 2, env=env, trace_stats=True)[0]
    assert_same(ser, two, counters=RESULT + TRAVERSAL)
    # the timed frames' kernel (no per-visit counters) gives the same film
    assert_same(ser, render(product, monkeypatch, spec, 1, 1, env=env)[0])
    # the interleaved loop's counters are another loop's: the switch is live on this scene
    off = render(product, monkeypatch, spec, 0, 0, trace_stats=True)[0]
    assert_same(off, ser)
    assert (off[2]["node_visits"], off[2]["tri_tests"]) != (ser[2]["node_visits"], ser[2]["tri_tests"])
    # iteration 0 (the interleaved loop by default) on the lists as well changes no result either
    it0 = render(product, monkeypatch, spec, 1, 1, env={"YAFARAY_AMD_TRACE_DEFER_IT0": "1"}, trace_stats=True)[0]
    assert_same(ser, it0)


INELIGIBLE = {
    "transparent-shadows": (lambda: scenes.cornell_transparent_shadows(48, 36, spp=2), None),
    "global-memory": (lambda: cornell(True), {"YAFARAY_AMD_SCENE_LDS": "0"}),
}


@pytest.mark.parametrize("case", list(INELIGIBLE))
def test_ineligible_renders_launch_no_deferred_kernel(product, monkeypatch, case):
    make, env = INELIGIBLE[case]
    spec = make()
    a = render(product, monkeypatch, spec, 0, env=env, trace_stats=True)[0]
    b = render(product, monkeypatch, spec, 1, env=env, trace_stats=True)[0]
    assert_same(a, b, counters=RESULT + TRAVERSAL)
    assert a[2]["node_visits"] > 0
    if case == "global-memory":
        assert a[2]["scene_in_lds"] == 0
