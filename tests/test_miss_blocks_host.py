"""The host's proof that a 16x16-pixel block of the image cannot hit the clip box (vx_host.hpp classify_miss_blocks, reached
through vx_debug_classify_miss_blocks: pure CPU, no context).  Safety: no ray of a flagged block hits the box, slab-tested in
float64 at nine jitter positions per pixel; the cases in which nothing may be flagged; and one usefulness bound on the bench view,
so that a classifier that proves nothing does not pass."""
import ctypes as C

import numpy as np
import pytest

from tests import common

BENCH_CLIP = ((0.25, 0.0, 0.0), (1.0, 1.0, 0.75))
CLIPS = {"whole": ((0.0, 0.0, 0.0), (1.0, 1.0, 1.0)), "bench": BENCH_CLIP, "slab": ((0.1, 0.47, 0.2), (0.9, 0.5, 0.85))}
SIZES = ((203, 131), (64, 48))     # no multiple of 16: the edge blocks are ragged
# the jitter positions (jx, jy) of [0, 1]^2: corners, edge midpoints, centre (the device draws from [0, 1))
NINE = [(a, b) for a in (0.0, 0.5, 1.0) for b in (0.0, 0.5, 1.0)]


@pytest.fixture(scope="module")
def grid():
    return common.grid(*common.small_noise(32))


def _mat(a):
    return np.array(list(a), dtype=np.float64).reshape(4, 4).T      # VxParams holds column-major matrices


def hits(p, w, h):
    """(h, w) bool: some ray of the pixel, at one of the nine jitter positions, passes the slab test of ray_box_intersection --
    setup_world_ray and the test restated in float64"""
    vi, pi = _mat(p.camera_view_inv), _mat(p.camera_proj_inv)
    lo, hi = np.array(list(p.volume_aabb_min), float), np.array(list(p.volume_aabb_max), float)
    cam = vi @ np.array([0.0, 0.0, 0.0, 1.0])
    cam = cam[:3] / cam[3]
    py, px = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    any_hit = np.zeros((h, w), bool)
    for jx, jy in NINE:
        sx = (px + 0.5) / w + (2.0 * jx - 1.0) / w
        sy = (py + 0.5) / h + (2.0 * jy - 1.0) / h
        ndc = np.stack([2.0 * sx - 1.0, 2.0 * sy - 1.0, np.zeros_like(sx), np.ones_like(sx)], axis=-1)
        v = ndc @ pi.T
        v = np.concatenate([v[..., :3] / v[..., 3:], np.ones_like(v[..., :1])], axis=-1)
        wp = v @ vi.T
        d = wp[..., :3] / wp[..., 3:] - cam
        d /= np.linalg.norm(d, axis=-1, keepdims=True)
        with np.errstate(divide="ignore", invalid="ignore"):
            t0, t1 = (lo - cam) / d, (hi - cam) / d
        near = np.fmax(0.0, np.fmin(t0, t1).max(axis=-1))
        far = np.fmax(t0, t1).min(axis=-1)
        any_hit |= near <= far
    return any_hit


def block_any(mask):
    h, w = mask.shape
    nby, nbx = (h + 15) // 16, (w + 15) // 16
    pad = np.zeros((nby * 16, nbx * 16), bool)
    pad[:h, :w] = mask
    return pad.reshape(nby, 16, nbx, 16).any(axis=(1, 3))


def classify(lib, p, w, h):
    nby, nbx = (h + 15) // 16, (w + 15) // 16
    flags = np.full((nby, nbx), 7, np.uint8)
    n = C.c_uint32(99)
    assert lib.vx_debug_classify_miss_blocks(C.byref(p), w, h, flags.ctypes.data, C.byref(n)) == 0
    assert set(np.unique(flags)) <= {0, 1} and int(flags.sum()) == n.value
    return flags.astype(bool)


def params(grid, w, h, cam_pos, look_at, clip=BENCH_CLIP, **kw):
    return common.make_scene(grid, w, h, "dvr", cam_pos=cam_pos, look_at=look_at, clip_min=clip[0], clip_max=clip[1], **kw)[4]


def test_hook_is_declared_and_checks_its_arguments(native_lib):
    from volxel_amd import _abi
    assert "vx_debug_classify_miss_blocks" in _abi.declared_symbols("volxel_hip.h")
    assert native_lib.vx_debug_classify_miss_blocks(None, 64, 48, None, None) != 0


def test_no_ray_of_a_flagged_block_hits_the_box(native_lib, grid):
    """40 seeded cameras around the unit box x 3 clip boxes x 2 image sizes"""
    rng = np.random.default_rng(20240611)
    flagged = proved_views = 0
    for _ in range(40):
        u = rng.normal(size=3)
        pos = u / np.linalg.norm(u) * rng.uniform(0.8, 2.5)
        look = rng.uniform(-0.35, 0.35, size=3)
        for clip in CLIPS.values():
            for w, h in SIZES:
                p = params(grid, w, h, tuple(pos), tuple(look), clip)
                miss = classify(native_lib, p, w, h)
                hit = block_any(hits(p, w, h))
                assert not (miss & hit).any(), (pos, look, clip, (w, h), np.argwhere(miss & hit))
                flagged += int(miss.sum())
                proved_views += bool(miss.any())
    assert proved_views >= 120 and flagged >= 2000      # of 240 views: the sweep is not vacuous


FORCED = {
    "camera_inside": dict(cam_pos=(0.2, 0.1, 0.05), look_at=(0.2, 0.1, 1.0)),
    "box_behind": dict(cam_pos=(0.0, 0.0, -2.0), look_at=(0.0, 0.0, -3.0)),
    "orthographic": dict(cam_pos=(0.0, 0.0, -4.0), look_at=(0.0, 0.0, 0.0), ortho=0.1),
}


@pytest.mark.parametrize("case", sorted(FORCED) + ["corner_on_plane", "nan_matrix", "switched_off"])
def test_everything_may_hit(native_lib, grid, case, monkeypatch):
    w, h = SIZES[0]
    far = dict(cam_pos=(0.0, 0.0, -4.0), look_at=(0.0, 0.0, 0.0))     # a small box in the middle of the image
    p = params(grid, w, h, **far)
    assert classify(native_lib, p, w, h).sum() > 40                  # the view itself leaves plenty to prove
    if case in FORCED:
        p = params(grid, w, h, **FORCED[case])
    elif case == "corner_on_plane":
        # looking along +z from beside the box, in the plane of its four front corners
        lo, hi = list(p.volume_aabb_min), list(p.volume_aabb_max)
        cam = (hi[0] + 1.0, hi[1], lo[2])
        p = params(grid, w, h, cam_pos=cam, look_at=(cam[0], cam[1], cam[2] + 1.0))
    elif case == "nan_matrix":
        p.camera_view_inv[5] = float("nan")
    else:
        monkeypatch.setenv("VX_DVR_MISS", "0")
    assert classify(native_lib, p, w, h).sum() == 0


def test_it_proves_most_of_what_misses_on_the_bench_view(native_lib, grid):
    """The bench camera at 1920 x 1080 with the bench clip box, 8160 blocks: the float64 slab test finds no hit at any of the nine
    positions in 3271 of them, the classifier flags 3265 (0.998).  At least 0.8 is asked for: the 2-pixel gap costs a few blocks
    next to the box's outline, nothing else."""
    w, h = 1920, 1080
    p = params(grid, w, h, **common.BENCH_CAM)
    miss = classify(native_lib, p, w, h)
    free = ~block_any(hits(p, w, h))
    print(f"blocks {miss.size}, without a hit {int(free.sum())}, flagged {int(miss.sum())}")
    assert not (miss & ~free).any()
    assert free.sum() > 1000 and miss.sum() >= 0.8 * free.sum()
