"""Maximum- and minimum-intensity projection on the GPU (VX_MODE_MIP / VX_MODE_MINIP, DESIGN.md section 2 "projections"): every
layout against the NumPy restatement (tests/projection_ref.py) with tolerance 0, range skipping bit-exact, the LDS-window kernel
against render_generic and the launch shapes against each other bit for bit, device groups, the refusals and a full-size frame."""
import ctypes as C

import numpy as np
import pytest

from tests import common
from tests import projection_ref as PR
from tests.common import bits, frame, grid, renderer, small_noise

W, H = 96, 64
LAYOUTS = {k: common.LAYOUTS[k] for k in ("brickf32", "bricku8", "reference", "cellquad")}
MODES = ("mip", "minip")
SETTINGS = dict(volume_clip_min=(0.25, 0.0, 0.0), volume_clip_max=(1.0, 1.0, 0.75), dvr_step_voxels=0.5, dvr_jitter=False,
                dvr_skip_empty=False, max_samples=1 << 20)


@pytest.fixture(scope="module")
def noise():
    return grid(*small_noise(64))


@pytest.fixture(scope="module")
def ct():
    from volxel_amd import synth
    return grid(*synth.ct_phantom(64))


def _scene(g, mode, layout=None, size=(W, H), devices=None, **kw):
    r = renderer(g, layout, devices, mode, size, **SETTINGS)
    for k, v in kw.items():     # after the pinned ones: a test may set one of them again
        setattr(r.settings, k, v)
    return r


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_image_matches_reference(noise, layout, mode):
    r = _scene(noise, mode, layout=LAYOUTS[layout])
    try:
        img, c = frame(r)
        tf, L = r._tf
        want, n, ntf, rays = PR.projection_image(r._params, noise, tf, L, minip=mode == "minip")
    finally:
        r.close()
    assert np.array_equal(img, want), float(np.abs(img - want).max())
    assert c.samples == n and c.skip_steps == 0
    assert c.tf_samples == ntf and c.rays == rays
    assert float(img[..., :3].max()) > 0.0      # the projection shows something


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["brickf32", "bricku8"])
@pytest.mark.parametrize("scene", ["noise", "ct"])
def test_range_skipping_is_exact(request, scene, layout, mode):
    g = request.getfixturevalue(scene)
    r = _scene(g, mode, layout=LAYOUTS[layout])
    try:
        off, c_off = frame(r)
        r.settings.dvr_skip_empty = True
        on, c_on = frame(r)
    finally:
        r.close()
    assert np.array_equal(bits(on), bits(off))
    assert c_off.skip_steps == 0
    assert c_on.samples + c_on.skip_steps == c_off.samples
    assert c_on.tf_samples == c_off.tf_samples and c_on.rays == c_off.rays
    if scene == "ct" and mode == "mip":
        assert c_on.skip_steps > 0      # past the bone, the soft tissue cannot raise the maximum


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("layout", ["brickf32", "bricku8"])
def test_kernels_and_launch_shapes_agree(ct, monkeypatch, layout, mode):
    """jitter on, skipping on: the LDS-window kernel (66 frames: the two single preview frames, then two 32-frame launches that
    fold the running mean themselves; and 66 single frames) against render_generic (VX_DVR_KERNEL=generic, set before its
    context exists)"""
    kw = dict(dvr_jitter=True, dvr_skip_empty=True)
    r = _scene(ct, mode, layout=LAYOUTS[layout], **kw)
    try:
        a, ca = frame(r, 66, 32)
        b, cb = frame(r, 66, 1)
    finally:
        r.close()
    monkeypatch.setenv("VX_DVR_KERNEL", "generic")
    gr = _scene(ct, mode, layout=LAYOUTS[layout], **kw)
    try:
        g, cg = frame(gr, 66, 32)
    finally:
        gr.close()
    assert ca.max_launch_frames == 32 and cb.max_launch_frames == 1
    if layout == "brickf32":
        assert ca.merge_launches == 0      # the kernel folded the running mean itself
    assert np.array_equal(bits(a), bits(b))
    assert np.array_equal(bits(a), bits(g))
    assert ca.samples + ca.skip_steps == cb.samples + cb.skip_steps == cg.samples + cg.skip_steps
    assert cg.skip_steps == 0 and ca.tf_samples == cg.tf_samples


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_group_matches_one_context(ct, mode):
    kw = dict(dvr_jitter=True, dvr_skip_empty=True, size=(256, 192))
    one = _scene(ct, mode, **kw)
    grp = _scene(ct, mode, devices=[0, 0, 0], **kw)
    try:
        a, ca = frame(one, 32, 32)
        b, cb = frame(grp, 32, 32)
    finally:
        one.close()
        grp.close()
    assert np.array_equal(bits(a), bits(b))
    assert (ca.samples, ca.skip_steps, ca.rays, ca.tf_samples, ca.pixels) == \
        (cb.samples, cb.skip_steps, cb.rays, cb.tf_samples, cb.pixels)


@pytest.mark.gpu
def test_refusals(noise):
    from volxel_amd import _abi
    r = _scene(noise, "mip")
    try:
        lib, ctx = r._lib, r._ctx
        r.bind_uniforms()
        p = _abi.VxParams()
        C.memmove(C.byref(p), C.byref(r._params), C.sizeof(p))
        assert lib.vx_set_params(ctx, C.byref(p)) == 0
        p.dvr_shadow_stride = 2
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_shadow_stride" in lib.vx_last_error(ctx)
        p.dvr_shadow_stride = 0
        p.render_mode = _abi.MODE_MINIP
        p.dvr_step_voxels = 0.0
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_step_voxels" in lib.vx_last_error(ctx)
        p.dvr_step_voxels = 0.5
        p.dvr_max_steps = (1 << 24) + 1
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"dvr_max_steps" in lib.vx_last_error(ctx)
        p.dvr_max_steps = 1000
        p.render_mode = 7
        assert lib.vx_set_params(ctx, C.byref(p)) == 1 and b"unknown render mode" in lib.vx_last_error(ctx)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", MODES)
def test_full_size_ct(mode):
    """BASELINE config 2 (256^3 CT phantom) at 1920x1080, skipping on, on a centred 160 x 96 crop"""
    from volxel_amd import synth
    g = grid(*synth.ct_phantom(256))
    r = _scene(g, mode, size=(1920, 1080), dvr_skip_empty=True)
    try:
        img, c = frame(r)
        tf, L = r._tf
        win = (880, 492, 1040, 588)
        want, n, ntf, rays = PR.projection_image(r._params, g, tf, L, minip=mode == "minip", window=win)
    finally:
        r.close()
    x0, y0, x1, y1 = win
    assert np.array_equal(img[y0:y1, x0:x1], want[y0:y1, x0:x1])
    assert n > 0 and ntf == rays == (x1 - x0) * (y1 - y0)     # every ray of the crop crosses the phantom
    if mode == "mip":
        assert float(want[y0:y1, x0:x1, :3].max()) > 0.0 and c.skip_steps > 0
