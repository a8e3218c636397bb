"""How a device layout becomes resident, and what it holds however it got there: given at construction, switched with
set_layout, built on demand beside the primary one, rebuilt by a second upload, and built layer by layer behind the chunks of
a pipelined atlas copy.  Every path that ends on the same (layout, render mode) must give the same bits; every native layout
must match the reference textures within the tolerances of test_gpu_parity.py (2e-6 for DVR, 1e-5 for Phong); and the
refusals of a volume beyond a layout's index range must leave a context that takes the next upload."""
import re
from types import SimpleNamespace

import numpy as np
import pytest

from tests import common
from volxel_amd import synth
from volxel_amd.settings import BENCHMARK_SETTINGS

pytestmark = pytest.mark.gpu

MODES = ("dvr", "dvr_phong", "no_dda")
SIZE = (72, 56)
# the conditions of test_bricku8_equals_brickf32_bit_for_bit: jitter, its sample range; `bounces` fixed for no_dda
SETTINGS = dict(dvr_jitter=True, sample_range=(0.05645751953125, 1.0), bounces=1)


def _tol(mode):
    return 1e-5 if mode == "dvr_phong" else 2e-6


def _counts(c):
    return (c.samples, c.rays, c.grad_samples)


def _shot(r, mode):
    """one jittered frame of `mode`: (image, (samples, rays, grad_samples), every counter bricku8 shares with brickf32)"""
    r.settings.render_mode = mode
    img, c = common.frame(r)
    return img, _counts(c), (c.samples, c.rays, c.tf_samples, c.grad_samples, c.lane_slots)


def _upload(r, g):
    """g into the context r holds, with the settings common.renderer gives a new one"""
    r.setup_from_grid(g)
    r.restore_settings(BENCHMARK_SETTINGS)
    for k, v in SETTINGS.items():
        setattr(r.settings, k, v)


def _same(got, want, what):
    assert np.array_equal(got[0], want[0]), what
    assert got[1] == want[1], (what, got[1], want[1])


# ---- 1. every way to reach a layout gives the same bits ---------------------------------------------------------------------------
@pytest.fixture(scope="module")
def volumes():
    """noise with constant bricks, 37 x 70 x 130 voxels: three different extents, none a multiple of 8, on the smallest brick
    grid with three different counts -- 8 x 16 x 24, since the builder rounds the brick counts up to multiples of 8 (the range
    mipmaps) -- so that a swapped axis or a mix-up of the brick grid with cellquad's apron grid shows; and a second volume of
    another shape (16 x 8 x 8 bricks)"""
    v, sp = synth.value_noise(136, seed=17, zero_quantile=0.5)
    a = np.ascontiguousarray(v[:130, :70, :37])
    a[:8, :8, :16] = 0                                   # two bricks that are constant whatever the noise does
    w, _ = synth.value_noise(72, seed=23, zero_quantile=0.4)
    b = np.ascontiguousarray(w[:13, :27, :70])
    ga, gb = common.grid(a, sp), common.grid(b, sp)
    assert tuple(ga.indirection_size) == (8, 16, 24) and tuple(gb.indirection_size) == (16, 8, 8)
    rng = np.asarray(ga.range, dtype=np.uint16).reshape(-1, 2)
    assert (rng[:, 0] == rng[:, 1]).any() and (rng[:, 0] != rng[:, 1]).any()   # constant and stored bricks
    return ga, gb


@pytest.fixture(scope="module")
def base(volumes):
    """(a) the layout given at construction, a fresh context per (layout, mode): what every other path is compared with;
    for the second volume DVR alone"""
    ga, gb = volumes
    out = {}
    for layout in (0, 1, 2, 3, 4):
        for mode in MODES:
            r = common.renderer(ga, layout, size=SIZE, **SETTINGS)
            out[(layout, mode)] = _shot(r, mode)
            r.close()
        r = common.renderer(gb, layout, size=SIZE, **SETTINGS)
        out[("b", layout)] = _shot(r, "dvr")
        r.close()
    return out


@pytest.mark.parametrize("mode", MODES)
def test_every_native_layout_matches_the_reference_textures(base, mode):
    ref = base[(0, mode)][0]
    assert base[(0, mode)][1][0] > 1000                  # the frame samples the volume
    for layout in (1, 2, 3, 4):
        err = float(np.abs(base[(layout, mode)][0] - ref).max())
        print(f"layout {layout} {mode}: max-abs against layout 0 {err:.3e}")
        assert err <= _tol(mode), (layout, mode, err)


@pytest.mark.parametrize("mode", ["dvr", "dvr_phong"])
def test_bricku8_is_brickf32_bit_for_bit(base, mode):
    a, b = base[(2, mode)], base[(4, mode)]
    assert np.array_equal(a[0], b[0])
    assert a[2] == b[2], (a[2], b[2])


def test_set_layout_walk_equals_construction(volumes, base):
    """(b) one context created with layout 0, walked 1 -> 2 -> 4 -> 3 -> 0 after the upload"""
    r = common.renderer(volumes[0], 0, size=SIZE, **SETTINGS)
    for layout in (1, 2, 4, 3, 0):
        r.set_layout(layout)
        for mode in MODES:
            _same(_shot(r, mode), base[(layout, mode)], (layout, mode))
    r.close()


@pytest.mark.parametrize("layout,walk", [(3, ("dvr", "no_dda", "dvr_phong", "dvr")), (1, ("dvr", "dvr_phong", "dvr"))])
def test_on_demand_build_equals_construction(volumes, base, layout, walk):
    """(c) AUTO builds cellquad beside the bricks for no_dda; cellquad gets brickf32 built beside it for Phong"""
    r = common.renderer(volumes[0], layout, size=SIZE, **SETTINGS)
    for step, mode in enumerate(walk):
        _same(_shot(r, mode), base[(layout, mode)], (layout, step, mode))
    r.close()


@pytest.mark.parametrize("layout", [0, 1, 2, 3, 4])
def test_second_upload_and_back_equals_construction(volumes, base, layout):
    """(d) a second volume of another shape into the same context, then the first again"""
    ga, gb = volumes
    r = common.renderer(ga, layout, size=SIZE, **SETTINGS)
    _same(_shot(r, "no_dda"), base[(layout, "no_dda")], "before")   # (AUTO: cellquad resident when the next upload comes)
    _upload(r, gb)
    _same(_shot(r, "dvr"), base[("b", layout)], "second volume")
    _upload(r, ga)
    for mode in MODES:
        _same(_shot(r, mode), base[(layout, mode)], ("first again", mode))
    r.close()


# ---- 2. the pipelined upload ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def slab():
    """1024 x 1024 x 24 voxels, no brick of the data constant: 8 MiB per atlas layer, so a 16 MiB copy chunk holds 2 layers.
    The 3 x 128 x 128 stored bricks come behind the atlas's slot 0, which makes 4 atlas layers: two copy chunks, one layout
    build issued behind the first and one for the tail.  The builder rounds the brick grid up to 128 x 128 x 8, so brickf32 has
    8 layers and cellquad 9 apron layers, those above the data from constant bricks.  A 64^3 noise block tiled in x and y."""
    v, sp = synth.value_noise(64, seed=5, zero_quantile=0.5)
    block = np.ascontiguousarray(v[:24])
    block[::8, ::8, ::8] += 7                            # no brick is constant, whatever the noise does
    g = common.grid(np.tile(block, (1, 16, 16)), sp)
    assert tuple(g.indirection_size) == (128, 128, 8) and tuple(g.atlas_size) == (1024, 1024, 32)
    return g


@pytest.fixture(scope="module")
def slab_reference(slab):
    r = common.renderer(slab, 0, size=(96, 64), **SETTINGS)
    out = _shot(r, "dvr")
    r.close()
    assert out[1][0] > 1000
    return out


@pytest.mark.parametrize("layout", [1, 2, 4])
def test_layers_built_behind_the_atlas_copy(slab, slab_reference, layout):
    prod = lambda t: int(t[0]) * int(t[1]) * int(t[2])
    r = common.renderer(slab, layout, size=(96, 64), **SETTINGS)
    seconds, nbytes, _ = r.upload_stats()
    want = prod(slab.atlas_size) + prod(slab.indirection_size) * 8 + sum(prod(s) for _, s in slab.range_mipmaps) * 4
    assert nbytes == want and seconds > 0.0
    img, _, _ = _shot(r, "dvr")
    r.close()
    err = float(np.abs(img - slab_reference[0]).max())
    print(f"layout {layout}: max-abs against layout 0 {err:.3e}, upload {seconds:.4f} s")
    assert err <= _tol("dvr"), (layout, err)


# ---- 3. the refusals of a volume beyond a layout's index range ----------------------------------------------------------------------
# brickf32 indexes 16-byte units with 32 bits (n_vox / 4 > 0xffffffff), bricku8 dwords (n_bricks * 128 > 0xfffffff0): with 512
# voxels a brick both are first exceeded by 2^25 bricks, here 512 x 512 x 128 of them, all constant -- no atlas, and the
# refusal comes before the layout's 64 GiB would be asked for.
BRICKS = (512, 512, 128)
N_BRICKS = BRICKS[0] * BRICKS[1] * BRICKS[2]
assert N_BRICKS * 512 // 4 > 0xffffffff and (N_BRICKS - 1) * 512 // 4 <= 0xffffffff
assert N_BRICKS * 128 > 0xfffffff0 and (N_BRICKS - 1) * 128 <= 0xfffffff0


@pytest.fixture(scope="module")
def constant_grid():
    bx, by, bz = BRICKS
    mip = lambda k: (bx >> k, by >> k, bz >> k)
    return SimpleNamespace(
        indirection=np.zeros(N_BRICKS, dtype=np.uint32), indirection_size=BRICKS,
        range=np.zeros(2 * N_BRICKS, dtype=np.uint16), range_size=BRICKS,
        atlas=np.zeros(0, dtype=np.uint8), atlas_size=(bx * 8, by * 8, 0),
        range_mipmaps=[(np.zeros(2 * mip(k)[0] * mip(k)[1] * mip(k)[2], dtype=np.uint16), mip(k)) for k in (1, 2, 3)],
        index_extent=(bx * 8, by * 8, bz * 8), min_maj=(0.0, 1.0), transform=np.eye(4, dtype=np.float32).reshape(-1))


@pytest.mark.parametrize("layout,message", [
    (2, f"volume too large for the brickf32 layout ({N_BRICKS * 512} voxels): select VX_LAYOUT_REFERENCE with vx_set_layout"),
    (4, f"volume too large for the bricku8 layout ({N_BRICKS} bricks): select VX_LAYOUT_REFERENCE with vx_set_layout")])
def test_volume_beyond_the_brick_index_range_is_refused(constant_grid, layout, message):
    from volxel_amd import Volxel3DRenderer, VolxelError
    r = Volxel3DRenderer(64, 64, layout=layout)
    with pytest.raises(VolxelError, match="^" + re.escape(message) + "$"):
        r.setup_from_grid(constant_grid)
    with pytest.raises(VolxelError, match="without a volume|no volume"):
        r.render()
    r.set_layout(0)                                      # the reference textures have no such limit
    r.setup_from_grid(constant_grid)
    assert r.upload_stats()[1] >= N_BRICKS * 8
    r.close()
