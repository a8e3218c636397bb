"""The segment views' restatement (tests/segview_ref.py) against closed forms, on the CPU: the masked volume voxel by voxel, two
blobs in disjoint bricks (ONLY(A) and HIDE(B) of A+B are A alone, for the projections, DVR and the isosurface), an empty and a
whole-volume segment, the ONLY / HIDE pair, and a wrong model -- masking after the trilinear mix instead of at the taps -- that
must break the two-blob identity (negative control).  Plus the ABI surface the hosts bind."""
import os
import re

import numpy as np
import pytest

from oracle import np_oracle as NP
from tests import iso_ref as IR
from tests import projection_ref as PR
from tests import segview_ref as SV

from tests.common import F32, ROOT, oracle_grid


@pytest.fixture(scope="module")
def two():
    ab, a, _ = SV.blobs()
    x = np.arange(ab.shape[2])[None, None, :]
    return {"ab": oracle_grid(ab), "a": oracle_grid(a), "raw": ab, "seg_a": (ab > 0) & (x < 24), "seg_b": (ab > 0) & (x >= 32)}


def _coords(shape):
    Z, Y, X = shape
    z, y, x = np.meshgrid(np.arange(-1, Z + 1), np.arange(-1, Y + 1), np.arange(-1, X + 1), indexing="ij")
    return x, y, z


def _scene(g, mode, w=32, h=24):
    from tests.common import benchmark_tf, make_scene
    tf, L = benchmark_tf()
    p = make_scene(g, w, h, mode, cam_pos=(0.3, 0.2, -1.0), sample_range=(0.0, 1.0))[4]   # both blobs in the sample range
    return p, tf, L


def test_masked_voxels_read_zero_and_the_rest_is_untouched(two):
    g, raw = two["ab"], two["raw"]
    plain = NP.NpVolume(g)
    keep = np.random.default_rng(3).random(raw.shape) < 0.5
    m = SV.MaskedVolume(g, keep)
    x, y, z = _coords(raw.shape)
    got, want = m.brick(x, y, z), plain.brick(x, y, z)
    inside = (x >= 0) & (y >= 0) & (z >= 0) & (x < raw.shape[2]) & (y < raw.shape[1]) & (z < raw.shape[0])
    k = np.zeros_like(inside)
    k[1:-1, 1:-1, 1:-1] = keep
    assert np.array_equal(got[inside & k], want[inside & k])
    assert not got[inside & ~k].any() and not np.signbit(got[inside & ~k]).any()   # +0.0f
    assert not got[~inside].any()


def test_only_and_hide_split_the_volume_exactly(two):
    g, seg = two["ab"], two["seg_a"]
    x, y, z = _coords(seg.shape)
    plain = NP.NpVolume(g).brick(x, y, z)
    only = SV.MaskedVolume(g, SV.visible(seg, "only")).brick(x, y, z)
    hide = SV.MaskedVolume(g, SV.visible(seg, "hide")).brick(x, y, z)
    assert np.array_equal(only + hide, plain)           # one of the two is +0 at every voxel: the sum is exact
    assert not (only * hide).any()


def test_empty_and_whole_segments(two):
    g, raw = two["ab"], two["raw"]
    x, y, z = _coords(raw.shape)
    plain = NP.NpVolume(g).brick(x, y, z)
    empty, whole = np.zeros(raw.shape, dtype=bool), np.ones(raw.shape, dtype=bool)
    assert not SV.MaskedVolume(g, SV.visible(empty, "only")).brick(x, y, z).any()
    assert np.array_equal(SV.MaskedVolume(g, SV.visible(empty, "hide")).brick(x, y, z), plain)
    assert np.array_equal(SV.MaskedVolume(g, SV.visible(whole, "only")).brick(x, y, z), plain)
    assert not SV.MaskedVolume(g, SV.visible(whole, "hide")).brick(x, y, z).any()
    p, tf, L = _scene(g, "mip")
    img = SV.projection_image(p, g, tf, L, empty, "only")[0]
    want = NP.transfer(tf, L, p.sample_range, np.zeros(1, dtype=F32))[0]   # m = 0 on every ray with a sample
    hit = PR.rays(p)[1] > 0
    assert hit.any() and np.array_equal(img[hit][:, :3], np.broadcast_to(want[:3] * want[3], (int(hit.sum()), 3)))


def test_two_blobs_only_a_and_hide_b_are_a_alone(two):
    ab, a = two["ab"], two["a"]
    x, y, z = _coords(two["raw"].shape)
    alone = NP.NpVolume(a).brick(x, y, z)
    assert np.array_equal(SV.MaskedVolume(ab, SV.visible(two["seg_a"], "only")).brick(x, y, z), alone)
    assert np.array_equal(SV.MaskedVolume(ab, SV.visible(two["seg_b"], "hide")).brick(x, y, z), alone)
    for mode, minip in (("mip", False), ("minip", True)):
        p, tf, L = _scene(ab, mode)
        want = PR.projection_image(p, a, tf, L, minip=minip)
        if not minip:   # (MinIP is 0 on every ray here: the blobs are surrounded by zeros)
            assert not np.array_equal(PR.projection_image(p, ab, tf, L, minip=minip)[0], want[0])   # B shows without a view
        for seg, view in ((two["seg_a"], "only"), (two["seg_b"], "hide")):
            got = SV.projection_image(p, ab, tf, L, seg, view, minip=minip)
            assert np.array_equal(got[0], want[0]) and got[1:] == want[1:], (mode, view)
    p, tf, L = _scene(ab, "dvr")
    want = NP.dvr_image(p, a, tf, L)
    for seg, view in ((two["seg_a"], "only"), (two["seg_b"], "hide")):
        got = SV.dvr_image(p, ab, tf, L, seg, view)
        assert np.array_equal(got[0], want[0]) and got[1] == want[1], view
    w_rgba, w_hit, w_counts, _ = IR.isosurface(p, a, 0.3)
    assert w_counts["hits"] > 0
    for seg, view in ((two["seg_a"], "only"), (two["seg_b"], "hide")):
        rgba, hit, counts, _ = SV.isosurface(p, ab, 0.3, seg, view)
        assert np.array_equal(hit, w_hit) and np.array_equal(rgba, w_rgba) and counts == w_counts, view


class _MaskAfterMix(NP.NpVolume):
    """WRONG model: the unmasked trilinear density, zeroed when the sample's nearest voxel is hidden (mask after the mix)"""

    def __init__(self, grid, keep):
        super().__init__(grid)
        self.keep = keep

    def trilinear_q(self, scale, qx, qy, qz):
        d = super().trilinear_q(scale, qx, qy, qz)
        i = [np.floor(np.asarray(q, dtype=F32) + F32(0.5)).astype(np.int64) for q in (qx, qy, qz)]
        ok = (i[0] >= 0) & (i[1] >= 0) & (i[2] >= 0) & (i[0] < self.ext[0]) & (i[1] < self.ext[1]) & (i[2] < self.ext[2])
        k = self.keep[np.where(ok, i[2], 0), np.where(ok, i[1], 0), np.where(ok, i[0], 0)]
        return np.where(ok & k, d, F32(0))


def test_negative_control_masking_after_the_mix_breaks_the_identity(two):
    ab, a = two["ab"], two["a"]
    p, tf, L = _scene(ab, "dvr")
    want = NP.dvr_image(p, a, tf, L)[0]
    keep = SV.visible(two["seg_a"], "only")
    plain = NP.NpVolume
    NP.NpVolume = lambda g: _MaskAfterMix(g, keep) if g is ab else plain(g)
    try:
        wrong = NP.dvr_image(p, ab, tf, L)[0]
    finally:
        NP.NpVolume = plain
    assert not np.array_equal(wrong, want)                 # the blob's rim: taps of hidden zeros mixed in, or not
    assert np.array_equal(SV.dvr_image(p, ab, tf, L, two["seg_a"], "only")[0], want)


def test_header_declares_the_views():
    h = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    enum = dict((k, int(v)) for k, v in re.findall(r"(VX_SEGVIEW_\w+) = (\d+)", h))
    assert enum == {"VX_SEGVIEW_OFF": 0, "VX_SEGVIEW_ONLY": 1, "VX_SEGVIEW_HIDE": 2}
    assert "int vx_set_segment_view(VxContext* ctx, int view);" in h
    assert "int vx_get_segment_view(VxContext* ctx, int* view);" in h


def test_library_refuses_a_view_without_a_context(native_lib):
    assert native_lib.vx_set_segment_view(None, 1) != 0
    assert native_lib.vx_get_segment_view(None, None) != 0


def test_hosts_carry_the_property():
    from volxel_amd import Volxel3DRenderer
    assert isinstance(Volxel3DRenderer.segment_view, property)
    assert Volxel3DRenderer.SEGMENT_VIEWS == ("off", "only", "hide")
    js = open(os.path.join(ROOT, "volxel_amd", "napi", "viewer.js")).read()
    assert "get segmentView()" in js and "set segmentView(view)" in js and "['off', 'only', 'hide']" in js
    dts = open(os.path.join(ROOT, "volxel_amd", "napi", "index.d.ts")).read()
    assert "segmentView: 'off' | 'only' | 'hide';" in dts
