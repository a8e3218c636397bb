"""The split DVR launch on the GPU: in a multi-frame launch the blocks the host proved cannot hit the
clip box run render_dvr_miss, the rest the LDS-window kernel; a single-frame launch is never split.  With VX_DVR_MISS=1 and =0,
each in a fresh context, the accumulated image is the same array bit for bit and every work counter is equal (kernel_ms,
last_kernel_ms and merge_ms are HIP-event times of two different runs and are left out).  The scene: the 32^3 noise volume at 203 x 131, the clip box over the middle third of the image
-- blocks that cannot hit, blocks with hits and misses, ragged edge blocks."""
import numpy as np
import pytest

from tests import common
from tests.common import frame, renderer

W, H = 203, 131
BLOCKS = 128 * 2            # 12 tiles of 64 x 64 pixels in groups of 8: the logical blocks of one frame
POS, LOOK = (1.9, 0.45, -2.4), (0.1, 0.0, -0.1)
TIMES = ("kernel_ms", "last_kernel_ms", "merge_ms")
SETTINGS = dict(volume_clip_min=(0.25, 0.0, 0.0), volume_clip_max=(1.0, 1.0, 0.75), max_samples=1 << 20)


@pytest.fixture(scope="module")
def noise():
    return common.grid(*common.small_noise(32))


def _scene(g, layout="brickf32", devices=None, pos=POS, look=LOOK, **kw):
    r = renderer(g, common.LAYOUTS[layout], devices, "dvr", (W, H), **{**SETTINGS, **kw})
    r.camera.pos, r.camera.view = np.asarray(pos, float), np.asarray(look, float)
    return r


def _work(c):
    return {name: getattr(c, name) for name, _ in c._fields_ if name not in TIMES}


def _both(monkeypatch, g, steps, **kw):
    """steps(r) -> list of (image, counters, blocks) in a fresh context under VX_DVR_MISS=1 and =0: ([...], [...])"""
    out = []
    for switch in ("1", "0"):
        monkeypatch.setenv("VX_DVR_MISS", switch)
        r = _scene(g, **kw)
        try:
            out.append(steps(r))
        finally:
            r.close()
    return out


def _shot(r, frames, in_flight):
    img, c = frame(r, frames, in_flight)
    return img, c, r.last_launch_blocks()


def _same(on, off):
    assert len(on) == len(off)
    for (a, ca, _), (b, cb, blocks_off) in zip(on, off):
        assert np.array_equal(a, b) and np.array_equal(common.bits(a), common.bits(b))
        assert _work(ca) == _work(cb)
        assert blocks_off[1] == 0          # VX_DVR_MISS=0: one kernel


# (frames, in_flight, frames of the largest launch): the two frames that follow a change go one by one and refresh the block order
LAUNCHES = {"fused32": (34, 32, 32), "fused64": (66, 64, 64), "unfused3": (5, 3, 3), "single": (3, 1, 1)}
VARIANTS = {
    "fused32": dict(), "fused64": dict(), "unfused3": dict(), "single": dict(),
    "jitter_off": dict(dvr_jitter=False), "environment_off": dict(show_environment=False),
    "jitter_off_environment_off": dict(dvr_jitter=False, show_environment=False),
    "bricku8": dict(layout="bricku8"), "skipping": dict(dvr_skip_empty=True), "bricku8_skipping": dict(layout="bricku8", dvr_skip_empty=True),
}


@pytest.mark.gpu
@pytest.mark.parametrize("case", sorted(VARIANTS))
def test_split_launch_is_bit_identical(noise, monkeypatch, case):
    """`single` covers weight 0 (frame 0) and weight != 0 (frames 1, 2): single-frame launches, which the switch must leave to the
    march kernel alone; the settings variants run the fused 32-frame launch and a 3-frame unfused one behind it"""
    kw = {"dvr_jitter": True, "show_environment": True, **VARIANTS[case]}
    shapes = [LAUNCHES[case]] if case in LAUNCHES else [LAUNCHES["fused32"], LAUNCHES["unfused3"]]

    def steps(r):
        return [_shot(r, n, fl) for n, fl, _ in shapes]
    on, off = _both(monkeypatch, noise, steps, **kw)
    _same(on, off)
    for (_, c, blocks), (n, _, largest) in zip(on, shapes):
        assert c.frames == n and c.max_launch_frames == largest
        if largest == 1:
            assert blocks == (BLOCKS, 0)
        else:
            assert blocks[0] + blocks[1] == BLOCKS and blocks[1] > BLOCKS // 2 and blocks[0] >= 12     # both kernels ran
        assert 0 < c.rays < c.pixels == n * W * H                  # hits and misses
    assert off[0][2] == (BLOCKS, 0)


@pytest.mark.gpu
def test_three_shards_gathered_and_detiled(noise, monkeypatch):
    def steps(r):
        return [_shot(r, 34, 32)]
    on, off = _both(monkeypatch, noise, steps, devices=[0, 0, 0], dvr_jitter=True)
    _same(on, off)
    one, _ = _both(monkeypatch, noise, steps, dvr_jitter=True)
    assert np.array_equal(on[0][0], one[0][0])
    assert _work(on[0][1])["pixels"] == _work(one[0][1])["pixels"] and on[0][1].rays == one[0][1].rays
    assert on[0][2][1] > 0


@pytest.mark.gpu
def test_camera_move_rebuilds_the_classification(noise, monkeypatch):
    """the camera turns upwards until the box has left the image, its corners still in front of the camera plane: every block is
    proved, the launch has no block for the LDS-window kernel at all (a single frame of that view still runs it alone); turned
    back, the first split returns"""
    pos = np.asarray(POS)
    d = -pos / np.linalg.norm(pos)
    side = np.cross(d, [0.0, 1.0, 0.0])
    up = np.cross(side / np.linalg.norm(side), d)
    away = pos + np.cos(np.radians(60.0)) * d + np.sin(np.radians(60.0)) * up

    def steps(r):
        out = [_shot(r, 34, 32)]
        r.camera.view = away
        out.append(_shot(r, 34, 32))
        out.append(_shot(r, 1, 1))
        r.camera.view = np.asarray(LOOK, float)
        out.append(_shot(r, 34, 32))
        return out
    on, off = _both(monkeypatch, noise, steps, dvr_jitter=True)
    _same(on, off)
    assert on[1][2] == (0, BLOCKS) and on[2][2] == (BLOCKS, 0) and on[1][1].rays == 0 and on[1][1].pixels == 34 * W * H
    assert on[0][2] == on[3][2] and on[0][2][0] > 0 and on[0][2][1] > 0
    assert np.array_equal(on[0][0], on[3][0])


@pytest.mark.gpu
def test_camera_inside_the_box_runs_the_march_kernel_alone(noise, monkeypatch):
    def steps(r):
        return [_shot(r, 34, 32), _shot(r, 2, 1)]
    on, off = _both(monkeypatch, noise, steps, pos=(0.1, 0.0, -0.1), look=(0.1, 0.0, 1.0), dvr_jitter=True)
    _same(on, off)
    assert on[0][2] == (BLOCKS, 0) and on[1][2] == (BLOCKS, 0)
    assert on[0][1].rays == on[0][1].pixels
