"""Renders with k_trace's flat scan (YAFARAY_AMD_TRACE_FLAT=1) against the deferred leaf lists (FLAT=0) and the
interleaved loop (YAFARAY_AMD_TRACE_DEFER=0): a Cornell render at 64 x 48 x 4 spp, depth 4, must give the same
film bits, weights, ray and sample counts with Russian roulette on and off, under the serial and the overlapped
schedule, with 2 / 5 / the default number of queue segments, twice on one Interface, and with iteration 0 on the
scan as well (YAFARAY_AMD_TRACE_FLAT_IT0=1).  The traversal's own counters (node visits = four leaf boxes each,
triangle tests) belong to the loop that ran: with FLAT=1 they are equal between the serial and the overlapped
schedule (a ray's tests depend on the ray and the scene alone) and differ from FLAT=0's, which shows that the
switch selects another loop."""
import numpy as np
import pytest

from libyafaray_amd import scenes
from test_trace_deferred_render import RESULT, TRAVERSAL, assert_same

pytestmark = pytest.mark.gpu

ENV = ("YAFARAY_AMD_TRACE_DEFER", "YAFARAY_AMD_TRACE_DEFER_CAP", "YAFARAY_AMD_TRACE_DEFER_IT0", "YAFARAY_AMD_TRACE_FLAT",
       "YAFARAY_AMD_TRACE_FLAT_IT0", "YAFARAY_AMD_OVERLAP", "YAFARAY_AMD_OVERLAP_SHADOW", "YAFARAY_AMD_SHADE_GRID", "YAFARAY_AMD_SCENE_LDS")
FLAT1 = {"YAFARAY_AMD_TRACE_FLAT": "1"}
FLAT0 = {"YAFARAY_AMD_TRACE_FLAT": "0"}
DEFER0 = {"YAFARAY_AMD_TRACE_DEFER": "0"}


def render(product, monkeypatch, spec, env, overlap=None, shade_grid=None, trace_stats=False, renders=1):
    """[(rgba, weights, stats)] of `renders` renders on one Interface under the given settings."""
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    if overlap is not None:
        monkeypatch.setenv("YAFARAY_AMD_OVERLAP", str(overlap))
    if shade_grid is not None:
        monkeypatch.setenv("YAFARAY_AMD_SHADE_GRID", str(shade_grid))
    for k, v in env.items():
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


def cornell(rr):
    return scenes.cornell(64, 48, spp=4, bounces=4, rr=rr)


@pytest.mark.parametrize("shade_grid", [2, 5, None])
@pytest.mark.parametrize("overlap", [0, 1])
@pytest.mark.parametrize("rr", [False, True])
def test_flat_render_equals_lists_and_interleaved(product, monkeypatch, rr, overlap, shade_grid):
    spec = cornell(rr)
    flat = render(product, monkeypatch, spec, FLAT1, overlap, shade_grid)[0]
    assert flat[2]["closest_rays"] > 0 and flat[2]["shadow_rays"] > 0
    assert_same(render(product, monkeypatch, spec, FLAT0, overlap, shade_grid)[0], flat)
    assert_same(render(product, monkeypatch, spec, DEFER0, overlap, shade_grid)[0], flat)
    assert_same(render(product, monkeypatch, spec, dict(FLAT1, YAFARAY_AMD_TRACE_FLAT_IT0="1"), overlap, shade_grid)[0], flat)


def test_flat_two_renders_on_one_interface(product, monkeypatch):
    spec = cornell(True)
    a = render(product, monkeypatch, spec, DEFER0)[0]
    b1, b2 = render(product, monkeypatch, spec, FLAT1, renders=2)
    assert_same(a, b1)
    assert_same(a, b2)


def test_flat_traversal_counters_do_not_depend_on_the_schedule(product, monkeypatch):
    spec = cornell(True)
    ser = render(product, monkeypatch, spec, FLAT1, 0, trace_stats=True)[0]
    ovl = render(product, monkeypatch, spec, FLAT1, 1, trace_stats=True)[0]
    assert_same(ser, ovl, counters=RESULT + TRAVERSAL)
    assert ser[2]["node_visits"] > 0 and ser[2]["tri_tests"] > 0
    two = render(product, monkeypatch, spec, FLAT1, 1, 2, trace_stats=True)[0]
    assert_same(ser, two, counters=RESULT + TRAVERSAL)
    # the timed frames' kernel (no per-visit counters) gives the same film
    assert_same(ser, render(product, monkeypatch, spec, FLAT1, 1)[0])
    # the lists' and the interleaved loop's counters are other loops': the switch is live on this scene
    lists = render(product, monkeypatch, spec, FLAT0, 0, trace_stats=True)[0]
    off = render(product, monkeypatch, spec, DEFER0, 0, trace_stats=True)[0]
    for other in (lists, off):
        assert_same(other, ser)
        assert (other[2]["node_visits"], other[2]["tri_tests"]) != (ser[2]["node_visits"], ser[2]["tri_tests"])
    # iteration 0 on the scan too: the same film, its own counters, schedule-independent as well
    it0 = dict(FLAT1, YAFARAY_AMD_TRACE_FLAT_IT0="1")
    s0 = render(product, monkeypatch, spec, it0, 0, trace_stats=True)[0]
    o0 = render(product, monkeypatch, spec, it0, 1, trace_stats=True)[0]
    assert_same(s0, o0, counters=RESULT + TRAVERSAL)
    assert_same(ser, s0)
    # an explicit list capacity asks for the lists: FLAT unset + CAP = the lists' counters at that capacity
    cap = {"YAFARAY_AMD_TRACE_DEFER_CAP": "8"}
    assert_same(lists, render(product, monkeypatch, spec, cap, 0, trace_stats=True)[0], counters=RESULT + TRAVERSAL)
