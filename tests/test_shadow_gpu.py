"""Shadowed DVR on the GPU (VxParams.dvr_shadow_stride, DESIGN.md section 2 "light grid"): the light grid and the shadowed image
against the NumPy restatement (tests/shadow_ref.py), launch shapes and device groups bit for bit, the rebuild rules, the
refusals, and a plausibility check against the reference's own one-bounce estimator."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import shadow_ref as SR
from tests.common import frame, renderer

W, H = 96, 64
LAYOUTS = {k: common.LAYOUTS[k] for k in ("brickf32", "bricku8", "reference", "cellquad")}
SETTINGS = dict(use_env=False, show_environment=False, volume_clip_min=(0.25, 0.0, 0.0), volume_clip_max=(1.0, 1.0, 0.75),
                dvr_shadow_stride=2, sync_light_dir=False, max_samples=1 << 20)


def _scene(g, layout=None, stride=2, size=(W, H), devices=None, **kw):
    return renderer(g, layout, devices, "dvr", size, **{**SETTINGS, "dvr_shadow_stride": stride}, **kw)


@pytest.fixture(scope="module")
def noise():
    from oracle import oracle as O
    from tests.common import small_noise
    vox, sp = small_noise(64)
    return O.BrickGrid(vox, sp)


LIGHTS = {"axis": (0.0, 0.0, -1.0), "oblique1": (-0.48, -0.6, -0.64), "oblique2": (0.8, -0.36, 0.48)}


@pytest.mark.gpu
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("light", sorted(LIGHTS))
def test_light_grid_matches_reference(noise, stride, light):
    r = _scene(noise, stride=stride, light_dir=LIGHTS[light])
    try:
        frame(r)
        got = r.read_shadow_grid()
        builds, light_samples, ms = r.shadow_stats()
        tf, L = r._tf
        want, n = SR.light_grid(r._params, noise, tf, L, stride)
    finally:
        r.close()
    assert builds == 1 and ms > 0.0
    assert got.shape == want.shape
    assert float(np.abs(got - want).max()) <= 2e-6
    assert light_samples == n and n > 0
    assert float(want.min()) < 0.5     # the light grid sees the volume


@pytest.mark.gpu
@pytest.mark.parametrize("ert", ["ert", "no_ert"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_shadowed_image_matches_reference(noise, layout, ert):
    """ert <= 0 (an epsilon >= 1) is served by render_generic's shadowed form on every layout; ert > 0 by the LDS-window kernel
    on brickf32 / bricku8"""
    eps = 1e-4 if ert == "ert" else 2.0
    r = _scene(noise, layout=LAYOUTS[layout], stride=2, dvr_ert_epsilon=eps, light_dir=LIGHTS["oblique1"])
    try:
        img, c = frame(r)
        r.settings.dvr_shadow_stride = 0
        plain, c0 = frame(r)
        tf, L = r._tf
        p = r._params
        p.dvr_shadow_stride = 2
        T, _ = SR.light_grid(p, noise, tf, L, 2)
        want, n, ntf = SR.dvr_image_shadowed(p, noise, tf, L, T, 2)
    finally:
        r.close()
    assert float(np.abs(img - want).max()) <= 1e-5
    assert (c.samples, c.rays, c.tf_samples) == (c0.samples, c0.rays, c0.tf_samples)
    assert c.samples == n and c.tf_samples == ntf
    assert float(np.abs(img - plain)[..., :3].max()) > 1e-3     # the shadow shows


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["brickf32", "bricku8"])
def test_launch_shapes_are_bit_identical(noise, layout):
    """jitter on: 64 frames at 32 per launch (the fused running mean) and 64 single-frame renders, skipping on and off"""
    imgs = []
    for skip in (True, False):
        r = _scene(noise, layout=LAYOUTS[layout], stride=2, dvr_jitter=True, dvr_skip_empty=skip)
        try:
            a, ca = frame(r, 64, 32)
            b, cb = frame(r, 64, 1)
        finally:
            r.close()
        assert ca.max_launch_frames == 32 and cb.max_launch_frames == 1
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), skip
        imgs.append(a)
    assert np.array_equal(imgs[0].view(np.uint32), imgs[1].view(np.uint32))


@pytest.mark.gpu
def test_group_matches_one_context(noise):
    one = _scene(noise, stride=2, size=(256, 192), dvr_jitter=True)
    grp = _scene(noise, stride=2, size=(256, 192), dvr_jitter=True, devices=[0, 0, 0])
    try:
        a, ca = frame(one, 32, 32)
        b, cb = frame(grp, 32, 32)
        assert grp.shadow_stats()[0] == 1 and grp.read_shadow_grid().shape == one.read_shadow_grid().shape
    finally:
        one.close()
        grp.close()
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert (ca.samples, ca.rays, ca.tf_samples, ca.pixels) == (cb.samples, cb.rays, cb.tf_samples, cb.pixels)


@pytest.mark.gpu
def test_rebuild_rules(noise):
    r = _scene(noise, stride=2, light_dir=LIGHTS["oblique1"])
    try:
        frame(r)
        assert r.shadow_stats()[0] == 1
        r.camera.pos = r.camera.pos + np.array([0.05, -0.02, 0.03])      # a camera move does not rebuild
        frame(r)
        frame(r)
        assert r.shadow_stats()[0] == 1
        r.settings.light_dir = LIGHTS["oblique2"]                       # light
        after_light, _ = frame(r)
        assert r.shadow_stats()[0] == 2
        cam = (r.camera.pos.copy(), r.camera.view.copy())
        tf, L = r._tf
        r.change_transfer_func(tf.copy(), L)                            # TF upload
        frame(r)
        assert r.shadow_stats()[0] == 3
        r.setup_from_grid(noise)                                        # volume upload
        r.settings.dvr_shadow_stride = 2
        frame(r)
        assert r.shadow_stats()[0] == 4
        r.settings.dvr_shadow_stride = 4                                # stride
        frame(r)
        assert r.shadow_stats()[0] == 5
    finally:
        r.close()
    fresh = _scene(noise, stride=2, light_dir=LIGHTS["oblique2"])      # after the light change: what a fresh context renders
    try:
        fresh.camera.pos, fresh.camera.view = cam
        want, _ = frame(fresh)
    finally:
        fresh.close()
    assert np.array_equal(after_light.view(np.uint32), want.view(np.uint32))


@pytest.mark.gpu
def test_refusals_and_path_modes_ignore_the_stride(noise):
    from volxel_amd import _abi
    r = _scene(noise, stride=0)
    try:
        lib, ctx = r._lib, r._ctx
        r.bind_uniforms()
        p = _abi.VxParams()
        C.memmove(C.byref(p), C.byref(r._params), C.sizeof(p))
        for bad in (3, -1, 8):
            p.dvr_shadow_stride = bad
            assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_shadow_stride" in lib.vx_last_error(ctx)
        p.dvr_shadow_stride = 2
        p.render_mode = _abi.MODE_DVR_PHONG
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_shadow_stride" in lib.vx_last_error(ctx)
        p.render_mode = _abi.MODE_DVR
        p.use_env = 1
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_shadow_stride" in lib.vx_last_error(ctx)
        p.use_env = 0
        assert lib.vx_set_params(ctx, C.byref(p)) == 0
        with pytest.raises(Exception):
            r.read_shadow_grid()      # nothing built yet
        r.settings.use_env = True
        r.settings.show_environment = True
        for mode in ("default", "no_dda", "raymarch"):
            r.settings.render_mode = mode
            r.settings.dvr_shadow_stride = 0
            a, ca = frame(r, 2, 1)
            r.settings.dvr_shadow_stride = 2
            b, cb = frame(r, 2, 1)
            assert np.array_equal(a.view(np.uint32), b.view(np.uint32)), mode
            assert (ca.samples, ca.rays) == (cb.samples, cb.rays), mode
        assert r.shadow_stats()[0] == 0
    finally:
        r.close()


def _plausibility_volume():
    """64^3: a receiver slab (index z in [4, 12), all x, y) and a dense occluder above it over x, y in [8, 32) (z in [36, 52))"""
    from oracle import oracle as O
    vox = np.zeros((64, 64, 64), dtype=np.uint16)
    vox[4:12, :, :] = 400
    vox[36:52, 8:32, 8:32] = 1000
    return O.BrickGrid(vox, (1.0, 1.0, 1.0))


@pytest.mark.gpu
def test_shadowed_dvr_is_closer_to_the_path_tracer():
    """The reference's raymarch mode (bounces = 1, directional light, no environment) converged over 384 frames on a 64 x 48
    image, seen from below the receiver slab with the light straight above the occluder.  Over the pixels the occluder
    shadows (shadowed / plain DVR < 0.8) the mean absolute difference to that mean must drop with the shadow term.  Margin from
    one MI355X run (2258 such pixels): plain DVR 0.2679, shadowed 0.0013; the test asks for less than a quarter of plain DVR's."""
    g = _plausibility_volume()
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer
    r = Volxel3DRenderer(64, 48, device=0)
    try:
        r.setup_from_grid(g)
        r.restore_settings(BENCHMARK_SETTINGS)
        tf = np.tile(np.array([1.0, 1.0, 1.0, 0.6], dtype=np.float32), 64)
        r.change_transfer_func(tf, 64)
        s = r.settings
        s.sample_range = (0.2, 1.0)
        s.use_env = False
        s.show_environment = False
        s.bounces = 1
        s.sync_light_dir = False
        s.light_dir = (0.0, 0.0, -1.0)
        s.volume_clip_min, s.volume_clip_max = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        r.camera.pos = np.array([0.05, 0.05, -1.3])
        r.camera.view = np.array([0.0, 0.0, 0.0])
        s.render_mode = "raymarch"
        s.max_samples = 100000
        mean, _ = frame(r, 384, 32)
        s.render_mode = "dvr"
        s.dvr_shadow_stride = 0
        plain, _ = frame(r)
        s.dvr_shadow_stride = 1
        shad, _ = frame(r)
    finally:
        r.close()
    lum = lambda im: im[..., :3].mean(axis=-1)
    region = (lum(shad) < 0.8 * lum(plain)) & (lum(plain) > 1e-3)
    assert region.sum() >= 50, region.sum()
    e_plain = float(np.abs(lum(plain) - lum(mean))[region].mean())
    e_shad = float(np.abs(lum(shad) - lum(mean))[region].mean())
    print(f"plausibility: {region.sum()} shadowed pixels, mean |DVR - raymarch| plain {e_plain:.4f} shadowed {e_shad:.4f}")
    assert e_shad < 0.25 * e_plain, (e_plain, e_shad)
