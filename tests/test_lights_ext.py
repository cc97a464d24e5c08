"""Spot, directional, sun and sphere lights on the GPU against the reference library's own pixels
(tests/golden/lights_ext.npz; scenes in lightslib.py): direct lighting, path tracing and photon mapping with
each light alone, and direct lighting and photon mapping with all of them beside the area light.

The bar is the project's 4 ULP per value.  The record comes from the reference's kd-tree, where an exact-t tie
between two primitives may resolve differently from this BVH, so at most 0.5 % of the pixels (8 of 1728) may
exceed it.  The control scenes (a point light) go through the same code and pass without the new lights."""
import dataclasses

import numpy as np
import pytest

import lightslib as LL
from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu

MAX_BAD = 8   # 0.5 % of 48 x 36 pixels


def _check(img, name):
    assert np.isfinite(img).all()
    ref = LL.fixture()[name]
    d = LL.ulp_distance(img, ref)
    bad = LL.bad_pixels(img, ref)
    print("%s: max %d ULP, %d values > 4 ULP, %d pixels > 4 ULP" % (name, int(d.max()), int((d > 4).sum()), bad))
    assert bad <= MAX_BAD, (name, bad, int(d.max()))


@pytest.mark.parametrize("name", LL.names())
def test_recorded_scene(product, name):
    rgba, _, _ = product.render_spec(LL.spec(name))
    _check(rgba, name)


def test_spot_in_several_chunks(product):
    rgba, _, _ = product.render_spec(LL.spec("spot_dl"), chunk_slots=1000)
    _check(rgba, "spot_dl")


def test_sun_device_group_equals_one_member(product):
    one, w1, _ = product.render_spec(LL.spec("sun_dl"))
    two, w2, _ = product.render_spec(LL.spec("sun_dl"), members=2)
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))
    assert np.array_equal(w1, w2)


@pytest.mark.parametrize("which", ["dir_inf", "sun"])
def test_unbounded_shadow_rays_cross_transparent_panes(product, which):
    """Shadow rays without an end (tmax = -1) through k_tshadow: the panes tint the light."""
    base = scenes.cornell_transparent_shadows(LL.W, LL.H, spp=2)
    # the light comes in through the open front: on their way out the shadow rays of the back wall and the floor
    # cross the panes and the two transparent boxes
    tinted = dataclasses.replace(base, lights=[LL.LIGHTS[which]])
    opaque = tinted.with_render(transp_shad=False)
    a, _, _ = product.render_spec(tinted)
    b, _, _ = product.render_spec(opaque)
    assert np.isfinite(a).all() and np.isfinite(b).all()
    assert a[..., :3].max() > 0
    assert not np.array_equal(a, b)


def test_path_tracing_all_lights_deferred_pick_equals_count_run(product, monkeypatch):
    """Path tracing with several lights resolves the light pick after the pass (k_dfr_nee) or in a count run
    (k_nee): both must hold the new lights' code and agree bit for bit."""
    spec = dataclasses.replace(LL.spec("all_dl"), render=LL.spec("spot_pt").render)
    monkeypatch.delenv("YAFARAY_AMD_LIGHT_PICK", raising=False)
    a, _, _ = product.render_spec(spec)
    monkeypatch.setenv("YAFARAY_AMD_LIGHT_PICK", "count")
    b, _, _ = product.render_spec(spec)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def _fg(spec, **kw):
    return spec.with_render(pm_final_gather=True, fg_samples=4, fg_bounces=2, **kw)


@pytest.mark.parametrize("which", LL.NEW + (LL.CONTROL,))
def test_final_gathering_is_finite_lit_and_near_the_photon_map_estimate(product, which):
    """Final gathering (the PhotonIntegrator's default) with each light, and with the control's point light through
    the same check.  The reference draws its radiance points
    with a racy random number, so no recorded pixels can serve.  The gathered image estimates the same radiance
    as the recorded render that reads the photon map directly; with 4 gather paths and a 20000-photon map both
    are noisy per pixel, but their means over the 1728 pixels are means of ~7000 gather paths and agree far
    inside a factor of two unless a light's in-place estimate is missing or counted twice."""
    rgba, _, _ = product.render_spec(_fg(LL.spec(which + "_pm")))
    assert np.isfinite(rgba).all()
    lit = int((rgba[..., :3].sum(-1) > 0).sum())
    ratio = float(rgba[..., :3].mean() / LL.fixture()[which + "_pm"][..., :3].mean())
    print("%s: final gathering lit %d pixels, mean / photon-map mean = %.3f" % (which, lit, ratio))
    assert lit > 400
    assert 0.5 < ratio < 2.0, ratio


def test_final_gathering_device_group_equals_one_member(product):
    spec = _fg(LL.spec("all_pm"))
    one, _, _ = product.render_spec(spec)
    two, _, _ = product.render_spec(spec, members=2)
    assert np.array_equal(one.view(np.uint32), two.view(np.uint32))


@pytest.mark.parametrize("integ", ["dl", "pm"])
def test_instanced_scene_built_on_the_device_has_the_scene_bound(product, monkeypatch, integ):
    """An infinite directional light and a sun take their position and radius from the scene bound.  An instanced
    scene whose BVH is built on the device takes it from the expansion's own reduction: the image equals the
    host build's, whose bound comes from the vertices read back (up to a BVH's exact-t ties, as above)."""
    spec = scenes.cornell_instanced(LL.W, LL.H, spp=2, bounces=3)
    spec = dataclasses.replace(spec, lights=[LL.LIGHTS["dir_inf"], LL.LIGHTS["sun"]], render=LL.spec("sun_" + integ).render)
    monkeypatch.setenv("YAFARAY_AMD_BVH_BUILD", "host")
    a, _, _ = product.render_spec(spec)
    monkeypatch.setenv("YAFARAY_AMD_BVH_BUILD", "gpu")
    b, _, _ = product.render_spec(spec)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    bad = LL.bad_pixels(b, a)
    print("instanced %s: %d pixels > 4 ULP between the device and the host build" % (integ, bad))
    assert bad <= MAX_BAD


# the kernels a render of the control scenes launched before these lights existed (kernel_times names, recorded on
# the commit before them)
OLD_KERNELS = {
    "dl": {"k_camera", "k_film", "k_nee", "k_shade", "k_trace"},
    "pt": {"k_camera", "k_film", "k_nee", "k_shade", "k_shade_staged", "k_trace"},
    "pm": {"k_camera", "k_film", "k_gather", "k_gather_walk", "k_nee", "k_photon_bounce", "k_photon_emit", "k_shade", "k_trace",
           "photon_compact", "pkd_build"},
}


@pytest.mark.parametrize("integ", ["dl", "pt", "pm"])
def test_old_lights_launch_no_new_kernel(product, integ):
    _, _, st = product.render_spec(LL.spec("bulb_" + integ), profile=True)
    names = set(st["kernel_times"])
    print(integ, sorted(names))
    assert names == OLD_KERNELS[integ], names ^ OLD_KERNELS[integ]


@pytest.mark.parametrize("name", ["spot_dl", "sun_pt", "ball_pm", "all_pm"])
def test_new_lights_run_the_xl_instantiations(product, name):
    """"k_lights_xl" counts the launches that ran an XL instantiation of k_nee, k_dfr_nee, k_photon_emit or k_fg:
    some with one of the new lights, none without (the exact sets above hold no such name)."""
    _, _, st = product.render_spec(LL.spec(name), profile=True)
    assert st["kernel_times"]["k_lights_xl"]["launches"] > 0
