"""Render layers (yafaray_defineLayer beyond "combined"): depth, normal, UV, barycentric, albedo and index layers.

Every in-scope layer is a closed-form function of the camera ray's first intersection that passes through the
combined image's film arithmetic, so the expected values never come from the code under test (layerlib.py):
* exact per pixel — 1 spp, box filter of width 1 (a sample's footprint is its own pixel): numpy values from the
  oracle-traced primitive, barycentrics and t of a numpy restatement of the camera;
* under real filtering — the oracle's *combined* render of an emissive twin that carries the layer's value as emission.
The bar is the project's image bar: <= 4 ULP per channel, no pixel excluded.
"""
import dataclasses

import numpy as np
import pytest

import filmfile
import layerlib as LL
import texscenes as TS
from libyafaray_amd import scenes

BAR = 4


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def render_layers(product, spec, members=None, chunk=None, cancel_after=None, callbacks=False):
    """Render `spec` (with spec.layers) through the C API: combined film, weights, {layer: film_layer()}, stats, and
    with callbacks the notify_layer calls and the put-pixel values per layer."""
    yi = product.Interface()
    scenes.apply(spec, yi)
    if members is not None:
        yi.set_device_group(members)
    if chunk:
        yi.L.yafaray_amd_setChunkSlots(yi.h, int(chunk))
    names = yi.layers()
    table = yi.layers_table()
    notes, px = [], {}
    seen = []

    def put(layer, x, y, r, g, b, a):
        px.setdefault(layer, np.full((spec.render.height, spec.render.width, 4), np.nan, np.float32))[y, x] = (r, g, b, a)

    def progress(total, done):
        seen.append(done)
        if cancel_after is not None and len([d for d in seen if d > 0]) >= cancel_after:
            yi.cancelRendering()

    kw = dict(put_layer_pixel=put, notify_layer=lambda *a: notes.append(a)) if callbacks else {}
    yi.render(progress=progress if cancel_after is not None else None, **kw)
    rgba, w = yi.film()
    films = {n: yi.film_layer(n) for n in names}
    st = yi.stats()
    yi.close()
    return dict(rgba=rgba, w=w, films=films, stats=st, names=names, table=table, notes=notes, px=px)


# ---- the machinery, on the CPU ----
def _exact_spec(**kw):
    return LL.layers_scene(37, 29, spp=1, tile=16, filter_type="box", pixelwidth=1.0, **kw)


def test_camera_restatement_matches_the_oracle(oracle_built):
    """The numpy camera's ray of every pixel hits the primitive whose colour the oracle's own 1-spp render of the
    emissive twin (one colour per primitive) shows there; misses show the black background."""
    spec = _exact_spec()
    n = len(spec.tris)
    col = np.stack([(np.arange(n) % 7 + 1) / 8.0, ((np.arange(n) // 7) % 7 + 1) / 8.0, (np.arange(n) // 49 + 1) / 16.0], -1).astype(np.float32)
    twin = LL.emissive_twin(spec, col)
    rgba, w, _ = oracle_built.OracleScene(twin, threads=4).render()
    hits = LL.first_hits(oracle_built, spec)
    want = np.where((hits["prim"] >= 0)[:, None], col[np.where(hits["prim"] >= 0, hits["prim"], 0)], 0.0).reshape(29, 37, 3)
    assert (hits["prim"] < 0).sum() > 20 and (hits["prim"] >= 0).sum() > 500
    assert len(np.unique(hits["prim"])) > 40
    assert np.array_equal(_bits(rgba[..., :3]), _bits(want))


def test_layer_spec_plumbing():
    """scenes.apply issues the defineLayer / index parameters (recorded by a stub API)."""
    calls = []

    class Stub:
        def __getattr__(self, name):
            return lambda *a: calls.append((name,) + a) or 1
    spec = dataclasses.replace(_exact_spec(), layers=[LL.layer("mist"), LL.layer("obj-index-abs", exported=None)])
    scenes.apply(spec, Stub())
    assert ("paramsSetString", "type", "mist") in calls and ("paramsSetInt", "object_index", 11) in calls
    assert ("paramsSetInt", "mat_pass_index", 7) in calls
    assert sum(1 for c in calls if c[0] == "defineLayer") == 3
    assert LL.TYPE_ORDER[0] == "combined" and sorted(LL.TYPE_ORDER[1:]) == sorted(LL.ALL_LAYERS)


# ---- 1. exact per pixel ----
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["prepass", "clip", "crop"])
def test_layers_exact_per_pixel(product, oracle_built, case):
    """37 x 29, tile 16 (ragged tiles), 1 spp, box 1.0.  prepass: farClip = -1 (the depth pre-pass' min / max);
    clip: near and far clip set, the back of the room beyond far; crop: xstart / ystart."""
    spec = _exact_spec()
    if case == "clip":
        spec = spec.with_camera(near_clip=3.0, far_clip=4.6)
    if case == "crop":
        spec = dataclasses.replace(spec.with_render(width=30, height=21, xstart=5, ystart=6))
    spec = dataclasses.replace(spec, layers=[LL.layer(n) for n in LL.ALL_LAYERS])
    want = LL.expected_layers(oracle_built, spec)
    hits = LL.first_hits(oracle_built, spec)
    assert (hits["prim"] < 0).any() and (hits["prim"] >= 0).any()
    if case == "clip":
        rays = LL.pixel_centre_rays(spec.with_camera(near_clip=0.0, far_clip=-1.0))
        open_hits = oracle_built.OracleScene(spec).trace_closest(rays)[1]
        assert ((open_hits >= 0) & (hits["prim"] < 0)).sum() > 50     # geometry beyond far / before near
    got = render_layers(product, spec)
    assert got["names"] == LL.TYPE_ORDER
    worst = {}
    for name in LL.ALL_LAYERS:
        g, e = got["films"][name], want[name]
        if name in ("obj-index-abs", "mat-index-abs"):
            e = np.ceil(e)
        if name in ("debug-normal-geom", "debug-normal-smooth", "debug-uv", "debug-barycentric-uvw", "adv-diffuse-color",
                    "obj-index-abs", "obj-index-norm", "mat-index-abs", "mat-index-norm"):
            e = e.copy()
            e[..., 3] = 1.0   # image types without alpha (Color, Gray) report alpha 1
        worst[name] = int(LL.ulp(g, e).max())
    print(case, worst)
    assert max(worst.values()) <= BAR, worst


# ---- 2. film arithmetic under real filtering ----
def _filtered(spec, filt=("gauss", 1.5)):
    return spec.with_render(width=41, height=23, aa_samples=5, filter_type=filt[0], aa_pixelwidth=filt[1], tile_size=8)


def _flat_scene(kind):
    if kind == "plain-mitchell4":
        # filterw clamped at 4.0: k_layer_film's generic window at 8 x 8 (reach 4 forward, 3 back), a signed table
        return _filtered(_flat_scene("plain"), ("mitchell", 4.0))
    if kind == "instanced":
        s = scenes.cornell_instanced(41, 23, spp=5, integrator="directlighting")
        objs = [dataclasses.replace(o, object_index=k) for o, k in zip(s.objects, (2, 0, 5, 1, 8, 13))]   # the base cube: 13
        mats = [dataclasses.replace(m, mat_pass_index=k) for m, k in zip(s.materials, (4, 1, 6))]
        s = dataclasses.replace(s, objects=objs, materials=mats)
    else:
        s = LL.layers_scene()
    s = dataclasses.replace(s.with_camera(resx=41, resy=23), normals=None)
    return _filtered(s)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "instanced", "plain-mitchell4"])
def test_index_layers_through_the_film(product, oracle_built, kind):
    spec = _flat_scene(kind)
    flat = scenes.flatten_instances(spec) if spec.instances else spec
    names = ["mat-index-norm", "obj-index-norm", "mat-index-abs", "obj-index-abs"]
    got = render_layers(product, dataclasses.replace(spec, layers=[LL.layer(n) for n in names]))
    oi, mi = LL.prim_object_index(flat), LL.prim_material_index(flat)
    oh = LL.highest(o.object_index for o in spec.objects)
    mh = LL.highest(m.mat_pass_index for m in spec.materials)
    if kind == "instanced":
        assert 13 in set(oi.tolist())   # the instances report their base's object_index
    vals = {"mat-index-norm": mi.astype(np.float32) / np.float32(mh), "obj-index-norm": oi.astype(np.float32) / np.float32(oh),
            "mat-index-abs": mi.astype(np.float32), "obj-index-abs": oi.astype(np.float32)}
    for n in names:
        twin, tw, _ = oracle_built.OracleScene(LL.emissive_twin(flat, vals[n][:, None]), threads=4).render()
        g = got["films"][n]
        assert np.array_equal(_bits(tw), _bits(got["w"]))
        if n.endswith("-abs"):
            assert np.array_equal(g[..., :3], np.ceil(twin[..., :3])), n
        else:
            assert int(LL.ulp(g[..., :3], twin[..., :3]).max()) <= BAR, n
        assert np.all(g[..., 3] == 1.0), n   # Gray: a type without alpha


def _albedo_scene(kind):
    if kind == "plain":
        s = _flat_scene("plain")
        mats = [dataclasses.replace(m, emit=m.diffuse_reflect) for m in s.materials]   # emission = albedo, same product
        return dataclasses.replace(s, materials=mats, lights=[])
    mats, imgs, tx = TS.case_clip_interp()
    mats = [dataclasses.replace(m, emit=1.0, params=dict(m.params, emit=TS.F(1.0))) for m in mats]
    s = TS.grid_scene(mats, imgs, tx, width=41, height=23, spp=5)
    # (the grid's own untextured floor emits its albedo too; a black background, as the layer's misses are)
    mats = [m if m.params is not None else dataclasses.replace(m, emit=m.diffuse_reflect) for m in s.materials]
    return dataclasses.replace(_filtered(s), lights=[], materials=mats, background=scenes.Background((0.0, 0.0, 0.0), 1.0))


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["plain", "texture-nodes"])
def test_diffuse_color_layer_through_the_film(product, oracle_built, kind):
    """adv-diffuse-color against the oracle's combined render of the scene's emissive twin: the same materials with
    emit = diffuse_reflect and no lights, whose radiance is emit x the diffuse shader's colour."""
    spec = _albedo_scene(kind)
    twin, tw, _ = oracle_built.OracleScene(spec, threads=4).render()
    got = render_layers(product, dataclasses.replace(spec, layers=[LL.layer("adv-diffuse-color", image_type="ColorAlpha")]))
    g = got["films"]["adv-diffuse-color"]
    assert np.array_equal(_bits(tw), _bits(got["w"]))
    assert (twin[..., :3] > 0).any()
    assert int(LL.ulp(g[..., :3], twin[..., :3]).max()) <= BAR
    hit = twin[..., 3] >= 1.0
    assert hit.sum() > 100 and int(LL.ulp(g[hit][:, 3], np.ones(hit.sum(), np.float32)).max()) <= 1


# ---- 3. combined is untouched ----
FOUR = ["z-depth-norm", "debug-normal-smooth", "adv-diffuse-color", "obj-index-abs"]


@pytest.mark.gpu
@pytest.mark.parametrize("integrator", ["directlighting", "pathtracing", "photonmapping"])
def test_combined_is_bit_identical_with_layers(product, integrator):
    spec = LL.layers_scene(48, 36, spp=2, tile=16, focal=1.2)
    spec = spec.with_render(integrator=integrator, bounces=3, rr_min_bounces=3, pm_photons=20000, pm_search=20, pm_bounces=3,
                            filter_type="gauss", aa_pixelwidth=1.5)
    a, w, st = product.render_spec(spec)
    got = render_layers(product, dataclasses.replace(spec, layers=[LL.layer(n) for n in FOUR]))
    assert np.array_equal(_bits(got["w"]), _bits(w))
    assert np.array_equal(_bits(got["rgba"]), _bits(a))
    # the first-hit pass traces one closest ray per sample, the depth pre-pass one per camera pixel
    assert got["stats"]["closest_rays"] - st["closest_rays"] == 48 * 36 * 2 + 48 * 36
    assert got["stats"]["shadow_rays"] == st["shadow_rays"]


# ---- 4. other film modes, against the oracle's film of the same samples ----
def _mode_spec():
    """The layers scene as its own emissive twin: every material emits its albedo (emit = diffuse_reflect, the
    same float product) and there are no lights, so the *combined* image of direct lighting is the albedo layer.
    Product and oracle then take the same adaptive decisions (they read the same combined film), and the oracle's
    combined render is the expected adv-diffuse-color of any film mode."""
    s = LL.layers_scene(40, 30, spp=2, tile=8, focal=1.1).with_render(filter_type="gauss", aa_pixelwidth=1.5)
    mats = [dataclasses.replace(m, emit=m.diffuse_reflect) for m in s.materials]
    names = ("mist", "debug-uv", "adv-diffuse-color", "mat-index-abs", "obj-index-norm")
    return dataclasses.replace(s, materials=mats, lights=[], layers=[LL.layer(n) for n in names])


def _same_layers(a, b):
    return all(np.array_equal(_bits(a["films"][n]), _bits(b["films"][n])) for n in a["names"]) and a["names"] == b["names"]


def _check_modes_against_oracle(oracle, spec, got, index_twins=True):
    """`got` (a product render of `spec` in any film mode) against the oracle's renders with the same render settings
    (passes, thresholds, sample offsets): adv-diffuse-color against the combined render of the scene itself, and —
    where every pixel is resampled (threshold 0), so that the twins take the same adaptive decisions —
    obj-index-norm and mat-index-abs against the combined renders of their emissive twins.  <= 4 ULP, ceil() exact."""
    plain = dataclasses.replace(spec, layers=[])
    ref, rw, _ = oracle.OracleScene(plain, threads=4).render()
    assert np.array_equal(_bits(rw), _bits(got["w"]))
    assert int(LL.ulp(got["rgba"], ref).max()) <= BAR
    worst = {"adv-diffuse-color": int(LL.ulp(got["films"]["adv-diffuse-color"][..., :3], ref[..., :3]).max())}
    if index_twins:
        oi = LL.prim_object_index(plain).astype(np.float32) / np.float32(LL.highest(o.object_index for o in plain.objects))
        tw, tww, _ = oracle.OracleScene(LL.emissive_twin(plain, oi[:, None]), threads=4).render()
        assert np.array_equal(_bits(tww), _bits(got["w"]))
        worst["obj-index-norm"] = int(LL.ulp(got["films"]["obj-index-norm"][..., :3], tw[..., :3]).max())
        mi = LL.prim_material_index(plain).astype(np.float32)
        tw, tww, _ = oracle.OracleScene(LL.emissive_twin(plain, mi[:, None]), threads=4).render()
        assert np.array_equal(got["films"]["mat-index-abs"][..., :3], np.ceil(tw[..., :3]))
    print(worst)
    assert max(worst.values()) <= BAR, worst


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["every-pixel", "some-pixels"])
def test_layers_adaptive_passes(product, oracle_built, case):
    """Adaptive passes accumulate into the layer planes (k_layer_film's accumulate and flags modes, the pass's own
    records at the multi-pass sample positions).  every-pixel: 2 passes, threshold 0 — albedo and index layers against
    the oracle's 2-pass films.  some-pixels: 3 passes with a real threshold, only part of the film resampled — the
    albedo layer against the oracle's combined film of the same adaptive render."""
    if case == "every-pixel":
        spec = _mode_spec().with_render(aa_passes=2, aa_inc_samples=2, aa_threshold=0.0)
    else:
        spec = _mode_spec().with_render(aa_passes=3, aa_inc_samples=2, aa_threshold=0.02)
    got = render_layers(product, spec)
    n_pix = 40 * 30
    if case == "every-pixel":
        assert got["stats"]["samples"] == n_pix * 4
    else:
        assert n_pix * 2 < got["stats"]["samples"] < n_pix * 6   # some pixels resampled, not all
    _check_modes_against_oracle(oracle_built, spec, got, index_twins=case == "every-pixel")
    one = render_layers(product, spec.with_render(aa_passes=1))
    assert not _same_layers(got, one)


@pytest.mark.gpu
def test_layers_resume_film(product, oracle_built, tmp_path):
    """save after pass 1, load-save continues: the resumed render's layers equal the oracle's uninterrupted 2-pass films
    (and the product's uninterrupted render bit for bit); the film file holds 1 + L unnormalised layers in type order."""
    path = str(tmp_path / "lay")
    spec = _mode_spec().with_render(aa_passes=2, aa_inc_samples=2, aa_threshold=0.0)
    full = render_layers(product, spec)
    first = render_layers(product, spec.with_render(aa_threshold=1e30, film_load_save_mode="save", film_load_save_path=path))
    f1 = filmfile.read(filmfile.film_path(path))
    assert len(f1.layers) == 1 + 5
    assert first["names"] == ["combined", "adv-diffuse-color", "mat-index-abs", "mist", "obj-index-norm", "debug-uv"]
    for k, n in enumerate(first["names"]):
        g = first["films"][n]
        if n == "mat-index-abs":
            assert np.array_equal(g[..., :3], np.ceil(f1.normalized(k))[..., :3])
        elif n in ("debug-uv", "adv-diffuse-color", "obj-index-norm"):
            assert np.array_equal(_bits(g[..., :3]), _bits(f1.normalized(k)[..., :3]))
        else:
            assert np.array_equal(_bits(g), _bits(f1.normalized(k))), n
    again = render_layers(product, spec.with_render(film_load_save_mode="load-save", film_load_save_path=path))
    _check_modes_against_oracle(oracle_built, spec, again)
    assert np.array_equal(_bits(again["rgba"]), _bits(full["rgba"]))
    assert _same_layers(again, full)
    # a film with another layer count is refused: the render starts over
    other = render_layers(product, dataclasses.replace(spec, layers=spec.layers[:2]).with_render(
        film_load_save_mode="load-save", film_load_save_path=path))
    assert other["stats"]["samples"] == full["stats"]["samples"]


@pytest.mark.gpu
def test_layers_device_group(product, oracle_built):
    """3 logical members on one GPU: the layer planes travel with the film's bands."""
    spec = _mode_spec()
    one = render_layers(product, spec, members=1)
    three = render_layers(product, spec, members=3)
    assert np.array_equal(_bits(three["rgba"]), _bits(one["rgba"]))
    assert _same_layers(three, one)
    ad = spec.with_render(aa_passes=2, aa_inc_samples=2, aa_threshold=0.0)
    grouped = render_layers(product, ad, members=3)
    _check_modes_against_oracle(oracle_built, ad, grouped)
    assert _same_layers(grouped, render_layers(product, ad, members=1))


@pytest.mark.gpu
def test_layers_canceled_then_complete(product):
    """A render canceled between chunks leaves every layer pixel whose footprint sources were all rendered equal to
    the complete render's, and unrendered pixels empty; a complete render afterwards is unaffected."""
    spec = _mode_spec().with_render(width=40, height=30, aa_samples=4, tile_size=8, filter_type="box", aa_pixelwidth=1.0)
    full = render_layers(product, spec, chunk=1024)
    part = render_layers(product, spec, chunk=1024, cancel_after=2)
    assert 0 < part["stats"]["samples"] < full["stats"]["samples"]
    done = part["w"] == full["w"]
    none = part["w"] == 0
    assert done.sum() > 0 and none.sum() > 0
    for n in full["names"]:
        eq = (_bits(part["films"][n]) == _bits(full["films"][n])).all(-1)
        assert eq[done].all(), n   # (the full weight: every source of the pixel's footprint was rendered)
        assert np.all(part["films"][n][none][:, :3] == 0), n
    assert _same_layers(render_layers(product, spec, chunk=1024), full)


# ---- 5. C API ----
@pytest.mark.gpu
@pytest.mark.parametrize("tiles", [True, False])
def test_layer_callbacks_and_table(product, tiles):
    """tiles: the per-tile path (one GPU); else a 2-member device group, whose pixels are put in the whole-film flush."""
    spec = LL.layers_scene(37, 29, spp=1, tile=16)
    layers = [LL.layer("z-depth-abs", exported="GrayAlpha", name="Z"), LL.layer("debug-normal-geom", exported="Color", name="N"),
              LL.layer("mat-index-abs", exported="Gray", name="M"), LL.layer("debug-uv", exported=None),
              {"type": "ao"}, {"type": "obj-index-auto"}, {"type": "no-such-layer"}]
    spec = dataclasses.replace(spec, layers=layers)
    got = render_layers(product, spec, callbacks=True, members=None if tiles else 2)
    assert got["names"] == ["combined", "mat-index-abs", "debug-normal-geom", "debug-uv", "z-depth-abs"]
    assert got["table"].splitlines() == [
        "Combined\tcombined\tColorAlpha\t4\tColor + Alpha [4 channels]",
        "M\tmat-index-abs\tGray\t1\tGray [1 channel]",
        "N\tdebug-normal-geom\tColor\t3\tColor [3 channels]",
        "Z\tz-depth-abs\tGrayAlpha\t2\tGray + Alpha [2 channels]"]
    assert got["notes"] == [("combined", "Combined", 37, 29, 4), ("mat-index-abs", "M", 37, 29, 1),
                            ("debug-normal-geom", "N", 37, 29, 3), ("z-depth-abs", "Z", 37, 29, 2)]
    # every exported layer's pixels, equal to film_layer(); the internal layer is readable but fires no callback
    assert sorted(got["px"]) == sorted(["combined", "mat-index-abs", "debug-normal-geom", "z-depth-abs"])
    for n, img in got["px"].items():
        assert np.array_equal(_bits(img), _bits(got["films"][n])), n
    assert got["films"]["debug-uv"].shape == (29, 37, 4) and (got["films"]["debug-uv"][..., 3] == 1).all()
    m = got["films"]["mat-index-abs"]
    assert np.array_equal(m, np.ceil(m)) and set(np.unique(m[..., 0]).tolist()) <= {0.0, 3.0, 5.0, 7.0}


@pytest.mark.gpu
def test_out_of_scope_layer_warns_and_combined_only_is_unchanged(product):
    spec = scenes.cornell(32, 24, spp=1, bounces=2)
    logs = []
    yi = product.Interface()
    cb = product.LoggerCb(lambda lvl, t, d, msg, data: logs.append((lvl, msg.decode())))
    yi.L.yafaray_setLoggingCallback.argtypes = [product.C.c_void_p, product.LoggerCb, product.C.c_void_p]
    yi.L.yafaray_setLoggingCallback(yi.h, cb, None)
    scenes.apply(spec, yi)
    assert yi.layers() == ["combined"] and yi.layers_table() == "combined\tCombined\tColorAlpha\n"
    yi.paramsClearAll()
    yi.paramsSetString("type", "ao")
    yi.defineLayer()
    assert any("'ao' is not produced by the GPU core" in m for _, m in logs)
    assert yi.layers() == ["combined"] and yi.layers_table() == "combined\tCombined\tColorAlpha\n"
    notes = []
    yi.render(notify_layer=lambda *a: notes.append(a))
    assert notes == [("combined", "Combined", 32, 24, 4)]
    with pytest.raises(RuntimeError):
        yi.film_layer("ao")
    yi.close()


@pytest.mark.gpu
def test_layer_redefined_after_the_scene_was_built(product):
    """A layer first defined without a usable image type (not produced), the scene built and rendered, then redefined
    with one: the next render rebuilds the scene with the layers' attribute rows and produces the layer."""
    spec = dataclasses.replace(scenes.cornell(32, 24, spp=1, bounces=2, integrator="directlighting"),
                               layers=[LL.layer("debug-uv", image_type="NoSuchType")])
    yi = product.Interface()
    scenes.apply(spec, yi)
    assert yi.layers() == ["combined"]
    yi.render()
    yi.paramsClearAll()
    yi.paramsSetString("type", "debug-uv")
    yi.paramsSetString("image_type", "Color")
    yi.defineLayer()
    assert yi.layers() == ["combined", "debug-uv"]
    yi.render()
    uv = yi.film_layer("debug-uv")
    yi.close()
    assert (uv[..., :2] > 0).any() and (uv[..., 3] == 1).all()
