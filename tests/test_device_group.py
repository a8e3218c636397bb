"""Device groups (vx_create_group): one image rendered on several GPUs from one process.  The group handle goes through
the existing entry points; the vx_read_* calls gather every member's slab with the pointer-table de-tile kernel.

CPU: the symbol is exported and declared, bad arguments are refused before any device is touched, and the Python host
checks its arguments before any library call.  GPU: groups with repeated device ids (the same kernel and event chain
as distinct devices, with local pointers for peer ones) render bit-identical images and the same work counters as one
context; the calls a group cannot serve are refused; a sharded context's own read is unchanged; the JavaScript host
renders through a group; distinct devices run when more than one GPU is visible."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests.common import NAPI, ROOT
VX_ERR_INVALID = 1


# ---- CPU ------------------------------------------------------------------------------------------------------------

def test_create_group_is_declared_and_exported(native_lib):
    from volxel_amd import _abi
    assert "vx_create_group" in _abi.declared_symbols("volxel_hip.h")
    assert hasattr(native_lib, "vx_create_group")


def test_create_group_refuses_bad_arguments_before_touching_a_device(native_lib):
    ids = (C.c_int * 65)(*([0] * 65))
    out = C.c_void_p(1234)
    assert native_lib.vx_create_group(None, 1, C.byref(out)) == VX_ERR_INVALID and not out.value
    for n in (0, 65, -1):
        out = C.c_void_p(1234)
        assert native_lib.vx_create_group(ids, n, C.byref(out)) == VX_ERR_INVALID and not out.value
        assert b"1 <= n <= 64" in native_lib.vx_last_error(None)
    assert native_lib.vx_create_group(ids, 1, None) == VX_ERR_INVALID


def test_renderer_refuses_device_together_with_devices():
    from volxel_amd import Volxel3DRenderer
    with pytest.raises(ValueError):
        Volxel3DRenderer(device=0, devices=[0])
    with pytest.raises(ValueError):
        Volxel3DRenderer(devices=[0, 0], shard_count=2)
    with pytest.raises(ValueError):
        Volxel3DRenderer(devices=[])


# ---- GPU ------------------------------------------------------------------------------------------------------------

W, H = 1920, 1080
# render mode, frames, frames per launch: DVR with fused 32-frame launches, the others a few frames each
MODES = [("dvr", 64, 32), ("dvr_phong", 8, 8), ("default", 3, 3), ("no_dda", 3, 1), ("raymarch", 3, 3)]


@pytest.fixture(scope="module")
def scene_msg():
    from volxel_amd import read_u16_stack_to_grid, synth
    vox, sp = synth.value_noise(256, seed=42)
    return read_u16_stack_to_grid(vox, sp)


def _renderer(msg, **kw):
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer
    r = Volxel3DRenderer(W, H, **kw)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.volume_clip_min = (0.25, 0.0, 0.0)
    r.settings.volume_clip_max = (1.0, 1.0, 0.75)
    return r


def _run(r, mode, frames, in_flight):
    r.settings.render_mode = mode
    r.restart_rendering()
    r.reset_counters()
    r.render(frames=frames, in_flight=in_flight)
    return r.read_accum(), r.counters()


@pytest.fixture(scope="module")
def single(scene_msg):
    r = _renderer(scene_msg, device=0)
    yield r
    r.close()


@pytest.fixture(scope="module")
def reference_images(single):
    """what one context renders, per mode: the yardstick of every group below"""
    return {m: _run(single, m, f, k) for m, f, k in MODES}


def _same_as_single(g, reference_images):
    for mode, frames, in_flight in MODES:
        img, c = _run(g, mode, frames, in_flight)
        want, wc = reference_images[mode]
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32)), mode
        assert (c.samples, c.rays, c.tf_samples, c.grad_samples) == \
            (wc.samples, wc.rays, wc.tf_samples, wc.grad_samples), mode
        assert c.frames == wc.frames == frames, mode
        if mode == "dvr":
            assert wc.samples > 0 and float(np.abs(want[..., :3]).max()) > 0.0


@pytest.mark.gpu
@pytest.mark.parametrize("devices", [[0, 0, 0], [0] * 8], ids=["x3", "x8"])
def test_group_of_repeated_ids_renders_like_one_context(scene_msg, single, reference_images, devices):
    g = _renderer(scene_msg, devices=devices)
    try:
        _same_as_single(g, reference_images)
        # the display pass reads the gathered image
        for r in (single, g):
            _run(r, "dvr", 32, 32)
        assert np.array_equal(g.read_display(), single.read_display())
        # balance_tiles: member 0 probes, every member gets the order; the image does not change
        perm = g.balance_tiles()
        assert sorted(perm.tolist()) == list(range(perm.size))
        img, c = _run(g, "dvr", 64, 32)
        want, wc = reference_images["dvr"]
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32))
        assert (c.samples, c.rays, c.tf_samples, c.frames) == (wc.samples, wc.rays, wc.tf_samples, wc.frames)
    finally:
        g.close()


@pytest.mark.gpu
def test_group_refuses_what_it_cannot_serve(scene_msg):
    from volxel_amd import VolxelError
    from volxel_amd.dist import slab_tensor
    g = _renderer(scene_msg, devices=[0, 0])
    lib, ctx = g._lib, g._ctx
    try:
        p = C.c_void_p()
        assert lib.vx_slab_device_ptr(ctx, C.byref(p)) == VX_ERR_INVALID and not p.value
        assert b"device group" in lib.vx_last_error(ctx)
        assert lib.vx_detile(ctx, C.c_void_p(16), C.c_void_p(16)) == VX_ERR_INVALID
        assert lib.vx_set_stream(ctx, None) == VX_ERR_INVALID
        with pytest.raises(VolxelError):
            slab_tensor(g)
        with pytest.raises(VolxelError):
            g.detile(16, 16)
        # params with their own sharding are refused; a member's error names the member and its device
        pp = g.bind_uniforms()
        pp.shard_count = 2
        assert lib.vx_set_params(ctx, C.byref(pp)) == VX_ERR_INVALID
        pp.shard_count, pp.render_mode = 1, 99
        assert lib.vx_set_params(ctx, C.byref(pp)) == VX_ERR_INVALID
        assert lib.vx_last_error(ctx).startswith(b"member 0 (device 0): ")
    finally:
        g.close()


@pytest.mark.gpu
def test_sharded_context_reads_its_own_tiles_like_the_torch_gather(scene_msg):
    """vx_read_accum of one shard (a table of its own slab and nulls) == the torch gather of that slab between zero
    slabs, de-tiled by vx_detile (the path of the per-process torch host)"""
    import torch
    from volxel_amd.dist import slab_tensor
    N = 3
    rr = _renderer(scene_msg, shard_rank=1, shard_count=N)
    try:
        _run(rr, "dvr", 4, 4)
        mine = rr.read_accum()
        slab = slab_tensor(rr).clone()
        gathered = torch.cat([torch.zeros_like(slab), slab, torch.zeros_like(slab)])
        image = torch.full((H * W * 4,), float("nan"), dtype=torch.float32, device="cuda")
        torch.cuda.synchronize()
        rr.detile(gathered.data_ptr(), image.data_ptr())
        rr.finish()
        want = image.view(H, W, 4).cpu().numpy()
        assert np.array_equal(mine.view(np.uint32), want.view(np.uint32))
        assert float(np.abs(mine).max()) > 0.0 and int((mine == 0).all(axis=2).sum()) > W * H // 2
    finally:
        rr.close()


@pytest.mark.gpu
def test_group_on_distinct_devices(scene_msg, reference_images):
    import torch
    visible = torch.cuda.device_count()
    if visible < 2:
        pytest.skip("one GPU visible: distinct-device groups need two or more")
    g = _renderer(scene_msg, devices=list(range(min(4, visible))))
    try:
        _same_as_single(g, reference_images)
    finally:
        g.close()


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_host_renders_through_a_group(tmp_path):
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "volxel_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    subprocess.check_call(["node", os.path.join(NAPI, "group_smoke.js"), str(tmp_path), "[0,0,0,0]"], timeout=300)
    res = json.load(open(tmp_path / "group.json"))
    assert res["devices"] == [0, 0, 0, 0]
    assert res["oneFrame"] is True and res["twelveFrames"] is True and res["nonzero"] is True
    assert res["frameIndex"] == 12 and res["samples"][0] == res["samples"][1] > 0
    assert "not both" in res["bothRefused"]
