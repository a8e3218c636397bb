"""Segmentation without a GPU (vx_segment, DESIGN.md section 2 "Segmentation"): the ABI of VxSegmentParams / VxSegmentResult and
the entry points, the refusals that need no device, mpr.overlay, and the NumPy / SciPy restatement (tests/segment_ref.py) held to
closed forms -- counts by integer enumeration, connectivity by construction -- each with a wrong model as a negative control
(6 taken for 26, an exclusive hi, a box off by one)."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from tests import segment_ref as SG
from tests.common import F32, F32_MAX, NAPI, ROOT
from tests.shapes import offsets, renderer_shell


# ---- the boundary ------------------------------------------------------------------------------------------------------
def test_segment_params_layout_matches_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxSegmentParams
    assert VxSegmentParams is _abi.VxSegmentParams
    names = [f[0] for f in VxSegmentParams._fields_]
    assert names == ["seed", "lo", "hi", "connectivity", "box_lo", "box_hi", "max_rounds"]
    got = offsets(tmp_path, "VxSegmentParams", names)
    assert got == [C.sizeof(VxSegmentParams)] + [getattr(VxSegmentParams, n).offset for n in names]
    assert got[0] == 4 * (3 + 2 + 1 + 3 + 3 + 1)


def test_segment_result_layout_matches_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxSegmentResult
    assert VxSegmentResult is _abi.VxSegmentResult
    names = [f[0] for f in VxSegmentResult._fields_]
    assert names == ["count", "bbox_lo", "bbox_hi", "d_min", "d_max", "d_sum", "rounds", "converged", "brick_visits"]
    got = offsets(tmp_path, "VxSegmentResult", names)
    assert got == [C.sizeof(VxSegmentResult)] + [getattr(VxSegmentResult, n).offset for n in names]
    assert got == [64, 0, 8, 20, 32, 36, 40, 48, 52, 56]


def test_segment_entry_points_are_declared_and_exported(native_lib):
    from volxel_amd import _abi
    for name in ("vx_segment", "vx_segment_read_mask", "vx_slice_segment_mask", "vx_segment_stats"):
        assert name in _abi.declared_symbols("volxel_hip.h")
        getattr(native_lib, name)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    invalid = int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))
    q, res, sp = _abi.VxSegmentParams(), _abi.VxSegmentResult(), _abi.VxSliceParams()
    bits = np.zeros(8, dtype=np.uint8)
    assert native_lib.vx_segment(None, C.byref(q), C.byref(res)) == invalid
    assert native_lib.vx_segment_read_mask(None, bits.ctypes.data, 8) == invalid
    assert native_lib.vx_slice_segment_mask(None, C.byref(sp), bits.ctypes.data) == invalid
    assert native_lib.vx_segment_stats(None, None, None, None) == invalid


def test_js_host_carries_the_segment_calls():
    c = open(os.path.join(NAPI, "volxel_napi.c")).read()
    js = open(os.path.join(NAPI, "viewer.js")).read()
    dts = open(os.path.join(NAPI, "index.d.ts")).read()
    for fn in ("vx_segment(", "vx_segment_read_mask(", "vx_slice_segment_mask(", "vx_segment_stats("):
        assert fn in c
    for m in ("segment(", "segmentMask(", "sliceMask(", "voxelIndex(", "segmentStats("):
        assert m in js and m in dts


# ---- Python-side refusals (no device: a renderer shell with a volume description) -------------------------------------
@pytest.mark.parametrize("kw, word", [
    (dict(seed=(16, 0, 0), lo=0.1), "seed"), (dict(seed=(0, 0, -1), lo=0.1), "seed"), (dict(seed=(0.5, 0, 0), lo=0.1), "seed"),
    (dict(seed=(0, 0), lo=0.1), "seed"), (dict(seed=(1, 1, 1), lo=float("nan")), "finite"),
    (dict(seed=(1, 1, 1), lo=0.1, hi=float("nan")), "finite"), (dict(seed=(1, 1, 1), lo=-math.inf), "finite"),
    (dict(seed=(1, 1, 1), lo=0.5, hi=0.4), "lo"), (dict(seed=(1, 1, 1), lo=0.1, connectivity=18), "connectivity"),
    (dict(seed=(1, 1, 1), lo=0.1, connectivity=True), "connectivity"),
    (dict(seed=(1, 1, 1), lo=0.1, box=((2, 0, 0), (1, 5, 5))), "box"), (dict(seed=(1, 1, 1), lo=0.1, box=((0, 0, 0), (16, 5, 5))), "box"),
    (dict(seed=(1, 1, 1), lo=0.1, box=((0, 0, 0), (0, 0, 24))), "box"), (dict(seed=(1, 1, 1), lo=0.1, box=(1, 2)), "box"),
    (dict(seed=(1, 1, 1), lo=0.1, max_rounds=-1), "max_rounds"), (dict(seed=(1, 1, 1), lo=0.1, max_rounds=2 ** 32), "max_rounds"),
])
def test_python_refusals(kw, word):
    with pytest.raises(ValueError, match=word):
        renderer_shell().segment(**kw)


def test_python_refusals_of_slice_mask_and_voxel_index():
    from volxel_amd import mpr
    r = renderer_shell()
    sp = mpr.axial(r, 3)
    sp.slab_samples = 0
    with pytest.raises(ValueError, match="slab_samples"):
        r.slice_mask(sp)
    with pytest.raises(TypeError):
        r.slice_mask("axial")
    with pytest.raises(ValueError, match="world_point"):
        r.voxel_index((0.0, float("nan"), 0.0))


def test_overlay_blends_only_the_mask():
    from volxel_amd import mpr
    img = np.zeros((4, 5, 4), dtype=np.uint8)
    img[..., 0], img[..., 3] = 100, 255
    m = np.zeros((4, 5), dtype=bool)
    m[1, 2] = True
    out = mpr.overlay(img, m, color=(0.0, 1.0, 0.0), alpha=0.25)
    assert out[1, 2].tolist() == [75, 64, 0, 255]          # (0.75 * 100, 0.25 * 255 + .5 floored, 0)
    keep = ~m
    assert np.array_equal(out[keep], img[keep]) and img[1, 2, 0] == 100
    assert np.array_equal(mpr.overlay(img, m, alpha=0.0), img)
    for bad in (dict(alpha=1.5), dict(color=(2, 0, 0)), dict(color=(1, 0))):
        with pytest.raises(ValueError):
            mpr.overlay(img, m, **bad)
    with pytest.raises(ValueError):
        mpr.overlay(img[..., 0], m)
    with pytest.raises(ValueError):
        mpr.overlay(img, m[:3])


# ---- the restatement against closed forms -----------------------------------------------------------------------------
def _ball(shape, c, r2):
    z, y, x = np.meshgrid(*[np.arange(n) for n in shape], indexing="ij")
    return (x - c[0]) ** 2 + (y - c[1]) ** 2 + (z - c[2]) ** 2 <= r2


def _lattice_count(r2):
    """integer points with x^2 + y^2 + z^2 <= r2, enumerated"""
    r = int(math.isqrt(r2))
    return sum(1 for x in range(-r, r + 1) for y in range(-r, r + 1) for z in range(-r, r + 1) if x * x + y * y + z * z <= r2)


@pytest.mark.parametrize("conn", [6, 26])
def test_two_disjoint_balls(conn):
    shape = (30, 28, 40)
    d = np.where(_ball(shape, (10, 12, 14), 36) | _ball(shape, (29, 14, 15), 25), F32(0.9), F32(0.1)).astype(F32)
    p = SG.predicate(d, 0.5, F32_MAX)
    a = SG.component(p, (10, 12, 14), conn)
    b = SG.component(p, (29, 14, 15), conn)
    assert a.sum() == _lattice_count(36) and b.sum() == _lattice_count(25)
    assert not (a & b).any()
    st = SG.stats(a, d)
    assert st["bbox_lo"] == (4, 6, 8) and st["bbox_hi"] == (16, 18, 20)
    assert st["d_min"] == st["d_max"] == float(F32(0.9)) and st["d_sum"] == math.fsum([float(F32(0.9))] * st["count"])
    assert not SG.component(p, (0, 0, 0), conn).any()            # a seed failing P: the empty set


def test_diagonal_chain_is_connected_under_26_only():
    shape = (12, 12, 12)
    d = np.zeros(shape, dtype=F32)
    for k in range(10):
        d[k, k, k] = 1.0          # corner neighbours
    d[9, 9, 10] = 1.0             # and one face step
    p = SG.predicate(d, 0.5, F32_MAX)
    assert SG.component(p, (0, 0, 0), 26).sum() == 11
    assert SG.component(p, (0, 0, 0), 6).sum() == 1               # negative control: 6 taken for 26 loses the chain
    # an edge-only chain
    e = np.zeros(shape, dtype=F32)
    for k in range(8):
        e[3, k, k] = 1.0
    pe = SG.predicate(e, 0.5, F32_MAX)
    assert SG.component(pe, (0, 0, 3), 26).sum() == 8 and SG.component(pe, (0, 0, 3), 6).sum() == 1


def test_shell_and_core_split_by_hi():
    shape = (24, 24, 24)
    core = _ball(shape, (12, 12, 12), 9)
    shell = _ball(shape, (12, 12, 12), 36) & ~core
    d = np.where(core, F32(0.8), np.where(shell, F32(0.5), F32(0.0))).astype(F32)
    n_core, n_all = _lattice_count(9), _lattice_count(36)
    both = SG.component(SG.predicate(d, 0.4, 0.8), (12, 12, 12), 6)
    shell_only = SG.component(SG.predicate(d, 0.4, 0.5), (12, 12, 18), 6)     # hi = 0.5 inclusive keeps the shell
    assert both.sum() == n_all and shell_only.sum() == n_all - n_core
    assert not SG.predicate(d, 0.4, 0.5)[12, 12, 12]                          # the core is out of the band
    # negative control: an exclusive hi loses the whole shell
    excl = (F32(0.4) <= d) & (d < F32(0.5))
    assert not excl.any()


def test_box_cuts_a_structure_in_two():
    shape = (8, 8, 32)
    d = np.zeros(shape, dtype=F32)
    d[4, 4, 2:30] = 1.0                                           # a rod along x from 2 to 29
    box = ((0, 0, 0), (15, 7, 7))                                 # x <= 15
    p = SG.predicate(d, 0.5, F32_MAX, box)
    seg = SG.component(p, (3, 4, 4), 6)
    assert seg.sum() == 14 and SG.stats(seg, d)["bbox_hi"] == (15, 4, 4)
    assert not SG.component(p, (20, 4, 4), 6).any()               # outside the box: P false, empty
    # negative control: the box one voxel short (an exclusive upper bound) loses x = 15
    short = SG.component(SG.predicate(d, 0.5, F32_MAX, ((0, 0, 0), (14, 7, 7))), (3, 4, 4), 6)
    assert short.sum() == 13


@pytest.mark.parametrize("conn", [6, 26])
def test_scipy_and_the_fixpoint_agree(conn):
    rng = np.random.default_rng(11)
    d = rng.random((14, 17, 19)).astype(F32)
    p = SG.predicate(d, 0.45, F32_MAX, ((1, 0, 2), (17, 15, 13)))
    seed = tuple(int(a) for a in np.argwhere(p)[0][::-1])
    a = SG.component(p, seed, conn)
    assert np.array_equal(a, SG.fixpoint(p, seed, conn))
    assert a.sum() > 1


def test_packing_round_trips():
    rng = np.random.default_rng(2)
    m = rng.random((8, 16, 24)) < 0.3
    bits = SG.packed(m)
    assert bits.size == m.size // 8
    assert np.array_equal(np.unpackbits(bits, bitorder="little").astype(bool).reshape(m.shape), m)
    assert np.array_equal(SG.unpacked(bits, m.shape), m)
    one = np.zeros((8, 8, 8), dtype=bool)
    one[0, 0, 1] = True
    assert SG.packed(one)[0] == 2                                 # LSB first, x fastest


def test_overlay_restatement_on_an_axial_plane():
    from volxel_amd import mpr
    rng = np.random.default_rng(3)
    m = rng.random((16, 16, 24)) < 0.4                            # (Z, Y, X)
    r = renderer_shell((24, 16, 16))
    sp = mpr.axial(r, 5)
    assert np.array_equal(SG.overlay(sp, m), m[5])
    sp.slab_samples, sp.dn[2] = 3, 1.0                            # a slab over z = 5, 6, 7
    assert np.array_equal(SG.overlay(sp, m), m[5] | m[6] | m[7])


def test_density_equals_trilinear_at_voxel_centres(native_lib):
    from oracle import np_oracle as NP
    from volxel_amd import read_u16_stack_to_grid, synth
    g = read_u16_stack_to_grid(*synth.value_noise(32, seed=4, zero_quantile=0.4))
    vol = NP.NpVolume(g)
    scale, inv_maj = F32(1.7), F32(0.61)
    d = SG.densities(vol, scale, inv_maj)
    X, Y, Z = vol.ext
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    t = vol.trilinear_q(scale, x.astype(F32), y.astype(F32), z.astype(F32)) * inv_maj
    assert np.array_equal(d.view(np.uint32), t.astype(F32).view(np.uint32))
    assert (d > 0).any()
