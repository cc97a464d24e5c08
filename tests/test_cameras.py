"""The architect, orthographic, equirectangular and angular cameras on the GPU against the reference library's own
pixels (tests/golden/cameras.npz; scenes in cameralib.py): direct lighting, path tracing and photon mapping, render
layers, the specular recursion tree, chunks, device groups, crop, and the samples the angular camera gives no ray.

The bar is the project's 4 ULP per value.  The record comes from the reference's kd-tree, where an exact-t tie
between two primitives may resolve differently from this BVH, so at most 0.5 % of the pixels (8 of 1728; 5 of the
equirectangular 1152) may exceed it: the cap and the reason of tests/test_lights_ext.py.  The control scene (the
perspective camera) goes through the same check."""
import dataclasses

import numpy as np
import pytest

import cameralib as CL
from libyafaray_amd import scenes

pytestmark = pytest.mark.gpu


def _max_bad(img):
    return (img.shape[0] * img.shape[1]) // 200   # 0.5 %: 8 of 48 x 36, 5 of 48 x 24


def _check(img, key, what=None):
    assert np.isfinite(img).all(), key
    ref = CL.fixture()[key]
    assert img.shape == ref.shape
    d = CL.ulp_distance(img, ref)
    bad = CL.bad_pixels(img, ref)
    print("%s: max %d ULP, %d values > 4 ULP, %d pixels > 4 ULP (cap %d)" % (what or key, int(d.max()), int((d > 4).sum()), bad, _max_bad(img)))
    assert bad <= _max_bad(img), (key, bad, int(d.max()))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _render_layers(product, spec):
    yi = product.Interface()
    scenes.apply(spec, yi)
    yi.render()
    rgba, _ = yi.film()
    films = {n: yi.film_layer(n) for n in yi.layers()}
    yi.close()
    return rgba, films


@pytest.mark.parametrize("name", [n for n in CL.names() if n not in CL.LAYERED])
def test_recorded_scene(product, name):
    rgba, _, _ = product.render_spec(CL.spec(name))
    _check(rgba, name)


@pytest.mark.parametrize("name", CL.circular_names())
def test_surround_is_exact(product, name):
    """Outside the circle every sample is the film's default colour: exact zeros and ones (and with a wide filter
    the same weights' sums as the record's), so the corners equal the record with no allowance."""
    rgba, _, _ = product.render_spec(CL.spec(name))
    ref = CL.fixture()[name]
    assert np.array_equal(_bits(CL.corners(rgba)), _bits(CL.corners(ref)))


def test_sample_without_ray_differs_from_a_miss(product):
    """Through the open front the wide angular camera sees the transparent background (alpha 0); outside its
    circle the pixels are black with alpha 1, although the same background stands behind them."""
    rgba, _, _ = product.render_spec(CL.spec("ang_wide_bg_dl"))
    assert np.array_equal(CL.corners(rgba), np.tile(np.float32([0, 0, 0, 1]), (4, 1)))
    assert (rgba[..., 3] == 0).sum() > 100


@pytest.mark.parametrize("name", CL.LAYERED)
def test_recorded_layers(product, name):
    """`combined` and the absolute depth, UV and smooth-normal layers: the depth is the hit distance along each
    camera ray, so it pins the rays themselves."""
    rgba, films = _render_layers(product, CL.spec(name))
    _check(rgba, name)
    for layer in CL.layer_names(name):
        _check(films[layer], name + "/" + layer)


@pytest.mark.parametrize("name", ["ang_equidistant_pt", "ortho_pt"])
def test_several_chunks_equal_one(product, name):
    one, w1, _ = product.render_spec(CL.spec(name))
    many, w2, _ = product.render_spec(CL.spec(name), chunk_slots=1000)
    assert np.array_equal(_bits(one), _bits(many))
    assert np.array_equal(w1, w2)


@pytest.mark.parametrize("name", ["ang_gauss_dl", "equi_pt"])
def test_device_group_equals_one_member(product, name):
    one, w1, _ = product.render_spec(CL.spec(name))
    for members in (2, 3):
        grp, w2, _ = product.render_spec(CL.spec(name), members=members)
        assert np.array_equal(_bits(one), _bits(grp)), members
        assert np.array_equal(w1, w2), members


def test_cropped_film_crosses_the_circle(product):
    """A crop window over the circle's edge (box filter, as tests/test_crop.py): away from the window's first row
    and column, whose pixels miss the splats from outside the film, it equals the full render's window."""
    full = CL.spec("ang_equidistant_dl")
    x0, y0, w, h = 2, 1, 22, 17   # the top-left corner region: outside, edge and inside of the circle
    a, wa, _ = product.render_spec(full)
    b, wb, _ = product.render_spec(full.with_render(width=w, height=h, xstart=x0, ystart=y0))
    sub = a[y0 + 1:y0 + h, x0 + 1:x0 + w]
    assert (sub == np.float32([0, 0, 0, 1])).all(-1).any() and (sub[..., :3].sum(-1) > 0).any()
    assert np.array_equal(_bits(sub), _bits(b[1:, 1:]))
    assert np.array_equal(wa[y0 + 1:y0 + h, x0 + 1:x0 + w], wb[1:, 1:])


def test_deferred_light_pick_equals_count_run(product, monkeypatch):
    """Two lights under path tracing: the light pick replays the one-thread order, in which a sample without a ray
    makes no pick, after the pass (the default) or in a count run."""
    spec = CL.spec("ang_two_lights_pt")
    monkeypatch.delenv("YAFARAY_AMD_LIGHT_PICK", raising=False)
    a, _, _ = product.render_spec(spec)
    monkeypatch.setenv("YAFARAY_AMD_LIGHT_PICK", "count")
    b, _, _ = product.render_spec(spec)
    assert np.isfinite(a).all() and a[..., :3].max() > 0
    assert np.array_equal(_bits(a), _bits(b))


@pytest.mark.parametrize("which", ["ortho", "equi"])
def test_final_gathering_is_finite_lit_and_near_the_photon_map_estimate(product, which):
    """Final gathering cannot be recorded (the reference draws its radiance points with a racy random number).  The
    gathered image estimates the same radiance as the recorded render that reads the photon map directly: with 4
    gather paths and a 20000-photon map both are noisy per pixel, but their means over the film are means of
    thousands of gather paths and agree far inside a factor of two (tests/test_lights_ext.py, the same check)."""
    spec = CL.spec(which + "_pm").with_render(pm_final_gather=True, fg_samples=4, fg_bounces=2)
    rgba, _, _ = product.render_spec(spec)
    assert np.isfinite(rgba).all()
    lit = int((rgba[..., :3].sum(-1) > 0).sum())
    ratio = float(rgba[..., :3].mean() / CL.fixture()[which + "_pm"][..., :3].mean())
    print("%s: final gathering lit %d pixels, mean / photon-map mean = %.3f" % (which, lit, ratio))
    assert lit > 400
    assert 0.5 < ratio < 2.0, ratio


def _kernels(product, name):
    _, _, st = product.render_spec(CL.spec(name), profile=True)
    return st["kernel_times"]


@pytest.mark.parametrize("name", ["ortho_dl", "equi_pt", "ang_equidistant_pt", "ang_square_dl", "ortho_pm"])
def test_other_cameras_run_the_xc_instantiation(product, name):
    kt = _kernels(product, name)
    assert kt["k_camera_xc"]["launches"] > 0
    assert "k_camera" not in kt


def test_perspective_and_architect_launch_the_perspective_kernels(product):
    control = _kernels(product, CL.CONTROL)
    arch = _kernels(product, "arch_dl")
    print(sorted(control))
    assert "k_camera_xc" not in control and control["k_camera"]["launches"] > 0
    assert set(arch) == set(control)


def test_architect_differs_from_perspective_on_the_tilted_camera(product):
    """The recorded architect scene looks down at the box: the same camera as `perspective` tilts the verticals."""
    rgba, _, _ = product.render_spec(CL.spec("arch_dl").with_camera(type="perspective"))
    assert np.isfinite(rgba).all()
    assert CL.bad_pixels(rgba, CL.fixture()["arch_dl"]) > 400


def test_circular_camera_with_normalised_depth_is_refused(product):
    import layerlib
    spec = dataclasses.replace(CL.spec("ang_equidistant_dl"), layers=[layerlib.layer("z-depth-norm")])
    yi = product.Interface()
    scenes.apply(spec, yi)
    with pytest.raises(RuntimeError) as e:
        yi.render()
    msg = str(e.value)
    assert "circular" in msg and "depth" in msg, msg
    assert yi.stats()["samples"] == 0   # nothing rendered
    yi.close()
