"""Intensity projections without a GPU (VX_MODE_MIP / VX_MODE_MINIP, DESIGN.md section 2 "projections"): the ABI of the two
modes and the bound entry point, both hosts carrying the modes, the NumPy restatement (tests/projection_ref.py) against closed
forms, and the density bounds of range skipping against every trilinear density a dense set of positions produces."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as NP
from tests import projection_ref as PR

from tests.common import F32, ROOT, oracle_grid


def test_header_modes_match_abi():
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    assert int(re.search(r"VX_MODE_MIP\s*=\s*(\d+)", text).group(1)) == _abi.MODE_MIP == 5
    assert int(re.search(r"VX_MODE_MINIP\s*=\s*(\d+)", text).group(1)) == _abi.MODE_MINIP == 6
    assert _abi.RENDER_MODES["mip"] == 5 and _abi.RENDER_MODES["minip"] == 6


def test_bound_entry_point_is_declared_and_exported(native_lib):
    from volxel_amd import _abi
    assert "vx_debug_build_projection_bounds" in _abi.declared_symbols("volxel_hip.h")
    getattr(native_lib, "vx_debug_build_projection_bounds")


@pytest.mark.parametrize("mode", ["mip", "minip"])
def test_settings_accept_and_round_trip_the_modes(mode):
    from volxel_amd import BENCHMARK_SETTINGS
    from volxel_amd.settings import verify_settings
    s = json.loads(json.dumps(BENCHMARK_SETTINGS))
    s["display"]["renderMode"] = mode
    verify_settings(s)
    back = json.loads(json.dumps(s))
    assert verify_settings(back)["display"]["renderMode"] == mode
    s["display"]["renderMode"] = "mipp"
    with pytest.raises(ValueError):
        verify_settings(s)


def test_renderer_exports_and_restores_the_mode(native_lib):
    from volxel_amd import ViewerSettings
    from volxel_amd.renderer import Volxel3DRenderer
    assert "render_mode" in Volxel3DRenderer.__dict__
    for mode in ("mip", "minip"):
        st = ViewerSettings(render_mode=mode)
        assert st.to_viewer_dict()["renderMode"] == mode


def test_js_render_mode_table_carries_the_modes():
    js = open(os.path.join(ROOT, "volxel_amd", "napi", "viewer.js")).read()
    table = re.search(r"const RenderMode = Object\.freeze\(\{([^}]*)\}\)", js).group(1)
    assert re.search(r"\bmip:\s*5\b", table) and re.search(r"\bminip:\s*6\b", table)
    dts = open(os.path.join(ROOT, "volxel_amd", "napi", "index.d.ts")).read()
    assert "mip: 5; minip: 6" in dts


def _tf():
    from tests.common import benchmark_tf
    return benchmark_tf()


@pytest.mark.parametrize("minip", [False, True])
def test_constant_volume_gives_tf_of_the_constant(minip):
    from tests.common import make_scene
    vox = np.full((64, 64, 64), 1000, dtype=np.uint16)   # (64^3: the index space is the data's)
    vox[0, 0, 0] = 4095      # outside the clip box: the constant normalises to 1000 / 4095, inside the sample range
    g = oracle_grid(vox)
    tf, L = _tf()
    s, cam, vol, ds, p = make_scene(g, 24, 16, "mip", sample_range=(0.0, 1.0), clip_min=(0.25, 0.25, 0.25),
                                    clip_max=(0.75, 0.75, 0.75))
    img, n, ntf, rays = PR.projection_image(p, g, tf, L, minip=minip)
    assert n > 0 and ntf == rays > 0
    c = NP.NpVolume(g).trilinear_q(p.volume_density_scale, F32(12.3), F32(13.7), F32(14.1)) * F32(p.volume_inv_maj)
    rgba = NP.transfer(tf, L, p.sample_range, np.asarray([c], dtype=F32))[0]
    want = rgba[:3] * rgba[3]
    hit = img[..., :3].any(axis=-1)
    assert hit.sum() == rays
    assert np.array_equal(img[hit][:, :3], np.broadcast_to(want, (int(hit.sum()), 3)))


def test_axis_ramp_under_the_ortho_camera_gives_its_last_and_first_samples():
    """a ramp rising along z, seen along +z by the orthographic camera: MIP shows the last sample of the ray, MinIP the first"""
    from tests.common import make_scene
    z = np.arange(64, dtype=np.float64)
    vox = np.broadcast_to((100 + 30 * z)[:, None, None], (64, 64, 64)).astype(np.uint16).copy()
    g = oracle_grid(vox)
    tf, L = _tf()
    s, cam, vol, ds, p = make_scene(g, 16, 16, "mip", cam_pos=(0.0, 0.0, -1.0), look_at=(0.0, 0.0, 0.0), ortho=0.2,
                                    sample_range=(0.0, 1.0), clip_min=(0.2, 0.2, 0.2), clip_max=(0.8, 0.8, 0.8))
    hit, n, q0, dq = PR.rays(p)
    assert hit.all() and abs(float(dq[2].flat[0])) > 0 and float(dq[0].flat[0]) == 0 and float(dq[1].flat[0]) == 0
    vol_np = NP.NpVolume(g)

    def dens(k):
        q = [NP.fma(np.asarray(k, dtype=F32), dq[i], q0[i]) for i in range(3)]
        return vol_np.trilinear_q(p.volume_density_scale, *q) * F32(p.volume_inv_maj)
    first, last = dens(F32(0)), dens(n - F32(1))
    rising = float(dq[2].flat[0]) > 0
    for minip, pick in ((False, last if rising else first), (True, first if rising else last)):
        img, *_ = PR.projection_image(p, g, tf, L, minip=minip)
        rgba = NP.transfer(tf, L, p.sample_range, pick)
        want = rgba[..., :3] * rgba[..., 3:]
        assert np.array_equal(img[..., :3], want)
    assert not np.array_equal(first, last)


def _bounds(lib, g, p):
    rng = np.asarray(g.range, dtype=np.uint16).view(np.uint32)
    bc = (C.c_uint32 * 3)(*g.indirection_size)
    level, dims = C.c_uint32(), (C.c_uint32 * 3)()
    assert lib.vx_debug_build_projection_bounds(rng.ctypes.data, bc, C.byref(p), None, C.byref(level), dims) == 0
    out = np.empty(2 * dims[0] * dims[1] * dims[2], dtype=F32)
    assert lib.vx_debug_build_projection_bounds(rng.ctypes.data, bc, C.byref(p), out.ctypes.data, C.byref(level), dims) == 0
    return out.reshape(dims[2], dims[1], dims[0], 2), int(level.value)


def _check_bounds(lib, g, p, per_axis=9):
    """every trilinear density of a dense lattice of cell-frame positions (per_axis per voxel, both ends of the index range
    included) lies within the bounds of its macro cell (mask index floor(q) + 1 >> (3 + level))"""
    b, level = _bounds(lib, g, p)
    ext = g.index_extent
    vol = NP.NpVolume(g)
    sh = 3 + level
    checked = 0
    for z0 in range(-1, ext[2] + 1, 4):
        zs = np.arange(z0, min(z0 + 4, ext[2] + 1), 1.0 / per_axis * 4)
        zz, yy, xx = np.meshgrid(zs, np.arange(-1, ext[1] + 1, 1.0 / per_axis * 4),
                                 np.arange(-1, ext[0] + 1, 1.0 / per_axis * 4), indexing="ij")
        q = [a.astype(F32).ravel() for a in (xx, yy, zz)]
        d = vol.trilinear_q(p.volume_density_scale, *q) * F32(p.volume_inv_maj)
        mi = [np.clip(np.floor(a).astype(np.int64) + 1, 0, e + 7) >> sh for a, e in zip(q, ext)]
        lo, hi = b[mi[2], mi[1], mi[0], 0], b[mi[2], mi[1], mi[0], 1]
        assert (d >= lo).all() and (d <= hi).all()
        checked += d.size
    assert np.isfinite(b).all() and (b[..., 0] <= b[..., 1]).all()
    return b, checked


def test_bounds_hold_on_small_noise(native_lib):
    from tests.common import make_scene, small_noise
    g = oracle_grid(*small_noise(64))
    p = make_scene(g, 8, 8, "mip")[4]
    b, n = _check_bounds(native_lib, g, p)
    assert n > 100000
    assert (b[..., 1] < b[..., 1].max()).any()      # the bounds differ between cells: they can skip


def test_bounds_hold_at_the_range_limits(native_lib):
    """bricks whose voxels sit on their range limits (codes 0 and 255 side by side), a full-scale density scale, and a tiny one"""
    from tests.common import make_scene
    rs = np.random.default_rng(5)
    vox = np.where(rs.random((48, 40, 56)) < 0.5, 0, 4095).astype(np.uint16)
    vox[:, :, :8] = 4095
    vox[20:, 8:16, :] = rs.integers(3000, 3100, size=vox[20:, 8:16, :].shape)
    g = oracle_grid(vox, (1.0, 1.0, 1.0))
    for mult in (1.0, 37.0, 1e-3):
        p = make_scene(g, 8, 8, "mip", density_multiplier=mult)[4]
        _check_bounds(native_lib, g, p, per_axis=5)


def test_bounds_do_not_skip_without_a_positive_scale(native_lib):
    from tests.common import make_scene, small_noise
    g = oracle_grid(*small_noise(32))
    p = make_scene(g, 8, 8, "mip")[4]
    p.volume_density_scale = 0.0
    b, _ = _bounds(native_lib, g, p)
    assert np.isneginf(b[..., 0]).all() and np.isposinf(b[..., 1]).all()
