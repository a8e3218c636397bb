"""Segment edits without a GPU (vx_segment_edit, vx_segment_write_mask; DESIGN.md section 2 "Segment edits"): the two
restatements of tests/segedit_ref.py (scipy.ndimage, and shifted copies in NumPy) against each other, against closed forms and
against the algebraic laws of the contract's border rules, each wrong model as a negative control on an input where it differs;
and the boundary: the symbols, VxSegmentEditParams, the Python refusals and the names of the JS host."""
import ctypes as C
import os
import re

import numpy as np
import pytest
from scipy import ndimage

from tests import segedit_ref as ER
from tests.common import ROOT
from tests.shapes import offsets, renderer_shell


# ---- the two restatements -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("n", [1, 2, 3, 5])
def test_scipy_and_shifted_copies_agree(conn, n):
    rng = np.random.default_rng(1)
    noise = rng.random((24, 32, 40)) < 0.3
    band = rng.random((24, 32, 40)) < 0.6
    blob = ER.blobs((24, 32, 40), seed=2)
    assert (noise & ~band).any()                      # M is not inside P
    for m in (noise, blob):
        for op in ER.OPS:
            assert np.array_equal(ER.scipy_edit(m, op, conn, n), ER.numpy_edit(m, op, conn, n)), op
        assert np.array_equal(ER.scipy_edit(m, "dilate", conn, n, band=band), ER.numpy_edit(m, "dilate", conn, n, band=band))


# ---- closed forms -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, count6", [(1, 7), (2, 25), (5, 231), (9, 1159)])
def test_one_voxel_dilated(n, count6):
    m = np.zeros((24, 24, 24), dtype=bool)
    m[12, 12, 12] = True
    assert count6 == (2 * n + 1) * (2 * n * n + 2 * n + 3) // 3
    assert int(ER.edit(m, "dilate", 6, n).sum()) == count6
    assert int(ER.edit(m, "dilate", 26, n).sum()) == (2 * n + 1) ** 3


@pytest.mark.parametrize("conn", [6, 26])
def test_cubes_erode_by_layers_but_not_from_outside_the_volume(conn):
    m = np.zeros((20, 20, 20), dtype=bool)
    m[4:15, 4:15, 4:15] = True                        # s = 11
    for n in (1, 2, 5):
        assert int(ER.edit(m, "erode", conn, n).sum()) == (11 - 2 * n) ** 3
    assert not ER.edit(m, "erode", conn, 6).any()
    f = np.zeros((20, 20, 20), dtype=bool)
    f[5:12, 6:13, 0:7] = True                         # pressed against the face x = 0
    e = ER.edit(f, "erode", conn, 2)
    assert int(e.sum()) == 3 * 3 * 5 and e[8, 9, 0] and e[:, :, 0].sum() == 9 and not e[:, :, 5:].any()
    whole = np.ones((9, 10, 11), dtype=bool)
    assert ER.edit(whole, "erode", conn, 4).all()


def _shell_with(channel):
    """a hollow 9^3 box near the face x = 0 of a 16^3 volume, its wall opened by `channel`"""
    m = ER.shell((16, 16, 16), (2, 3, 3), (10, 11, 11))
    assert int(m.sum()) == 9 ** 3 - 7 ** 3
    if channel == "straight":                         # one voxel through the wall x = 2, then the background to the face
        m[7, 7, 2] = False
    elif channel == "diagonal":                       # the wall x = 2 is two voxels thick here, opened by two voxels that
        m[6:9, 6:9, 3] = True                         # touch only across an edge
        m[7, 7, 3] = False
        m[7, 8, 2] = False
    return m


def test_fill_holes_closed_forms():
    solid = 9 ** 3
    for conn in (6, 26):
        assert int(ER.edit(_shell_with(None), "fill_holes", conn).sum()) == solid
        m = _shell_with("straight")
        assert np.array_equal(ER.edit(m, "fill_holes", conn), m)                   # open to the face: nothing is filled
    d = _shell_with("diagonal")
    f6, f26 = ER.edit(d, "fill_holes", 6), ER.edit(d, "fill_holes", 26)
    assert np.array_equal(f26, d)                                                   # open to 26
    assert int(f6.sum()) == solid - 1 and not f6[7, 8, 2]                           # closed to 6: all but the outer notch
    # negative control: the other connectivity on the same input differs
    assert not np.array_equal(f6, f26) and int((f6 ^ f26).sum()) == 7 ** 3 - 9 + 1


@pytest.mark.parametrize("conn", [6, 26])
def test_open_removes_a_one_voxel_bridge(conn):
    m = np.zeros((16, 16, 32), dtype=bool)
    m[4:11, 4:11, 3:10] = True
    m[4:11, 4:11, 20:27] = True
    m[7, 7, 10:20] = True
    o = ER.edit(m, "open", conn, 1)
    assert not (o & ~m).any()
    if conn == 26:
        assert not o[7, 7, 10:20].any() and int(o.sum()) == 2 * 7 ** 3          # the bridge goes, both cubes keep their count
    else:
        # the 6-neighbourhood is a cross: an opened cube keeps what a cross inside it covers (not its 8 corners and 12 edges of
        # 5), and the cross centred on the face voxel under each end of the bridge keeps that end's first voxel
        assert not o[7, 7, 11:19].any() and o[7, 7, 10] and o[7, 7, 19]
        assert int(o.sum()) == 2 * (7 ** 3 - 8 - 12 * 5) + 2
    assert ndimage.label(o)[1] == 2 and ndimage.label(m)[1] == 1


# ---- laws ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
@pytest.mark.parametrize("n", [1, 2, 4])
def test_laws_at_the_faces(conn, n):
    m = ER.blobs((20, 28, 36), seed=7)
    for a in range(3):
        assert m.take(0, axis=a).any() and m.take(-1, axis=a).any()
    cl, op = ER.edit(m, "close", conn, n), ER.edit(m, "open", conn, n)
    assert not (m & ~cl).any() and (cl & ~m).any()            # extensive, and it does something
    assert not (op & ~m).any() and (m & ~op).any()            # anti-extensive
    assert np.array_equal(ER.edit(cl, "close", conn, n), cl)
    assert np.array_equal(ER.edit(op, "open", conn, n), op)
    assert np.array_equal(ER.edit(m, "erode", conn, n), ~ER.edit(~m, "dilate", conn, n))
    # scipy's own closing, with its single border value, is not extensive at the faces: why the halves are composed
    sc = ndimage.binary_closing(m, ER.structure(conn), iterations=n)
    assert (m & ~sc).any()


# ---- negative controls --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("conn", [6, 26])
def test_wrong_models_differ(conn):
    # scipy's default border_value = 0 erodes a structure that touches a face from outside the volume
    f = np.zeros((20, 20, 20), dtype=bool)
    f[5:12, 6:13, 0:7] = True
    right = ER.edit(f, "erode", conn, 2)
    wrong = ndimage.binary_erosion(f, ER.structure(conn), iterations=2)
    assert right.any() and wrong.any() and (right ^ f).any()
    assert not np.array_equal(right, wrong) and not (wrong & ~right).any() and int(right.sum()) - int(wrong.sum()) == 3 * 3 * 2
    # the band applied once after n free steps, instead of at every step, crosses a wall that is not in P
    m = np.zeros((12, 12, 24), dtype=bool)
    m[4:8, 4:8, 2:6] = True
    band = np.ones_like(m)
    band[:, :, 8] = False                              # a wall of non-P voxels between the seed and the far side
    right = ER.edit(m, "dilate", conn, 6, band=band)
    wrong = m | (ER.edit(m, "dilate", conn, 6) & band)
    assert (right ^ m).any() and not right[:, :, 8:].any() and wrong[:, :, 9:].any()
    assert not np.array_equal(right, wrong)


# ---- the boundary -------------------------------------------------------------------------------------------------------
def test_edit_params_layout_matches_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxSegmentEditParams
    assert VxSegmentEditParams is _abi.VxSegmentEditParams
    names = [f[0] for f in VxSegmentEditParams._fields_]
    assert names == ["op", "connectivity", "steps", "band"]
    got = offsets(tmp_path, "VxSegmentEditParams", names)
    assert got == [C.sizeof(VxSegmentEditParams)] + [getattr(VxSegmentEditParams, n).offset for n in names]
    assert got == [16, 0, 4, 8, 12]


def test_enum_and_limits_match_the_header():
    from volxel_amd import _abi
    from volxel_amd.renderer import Volxel3DRenderer
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    for name, value in _abi.SEGEDIT_OPS.items():
        assert int(re.search(r"VX_SEGEDIT_%s = (\d+)" % name.upper(), text).group(1)) == value
    assert Volxel3DRenderer.SEGMENT_EDIT_OPS == tuple(sorted(_abi.SEGEDIT_OPS, key=_abi.SEGEDIT_OPS.get)) == ER.OPS
    assert int(re.search(r"#define VX_SEGEDIT_MAX_STEPS (\d+)u", text).group(1)) == _abi.SEGEDIT_MAX_STEPS == 1024


def test_entry_points_are_declared_and_exported(native_lib):
    from volxel_amd import _abi
    for name in ("vx_segment_edit", "vx_segment_write_mask", "vx_segment_edit_stats"):
        assert name in _abi.declared_symbols("volxel_hip.h")
        getattr(native_lib, name)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    invalid = int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))
    q, res = _abi.VxSegmentEditParams(), _abi.VxSegmentResult()
    bits = np.zeros(8, dtype=np.uint8)
    assert native_lib.vx_segment_edit(None, C.byref(q), C.byref(res)) == invalid
    assert native_lib.vx_segment_write_mask(None, bits.ctypes.data, 8, C.byref(res)) == invalid
    assert native_lib.vx_segment_edit_stats(None, None, None) == invalid


@pytest.mark.parametrize("kw, word", [
    (dict(op="grow"), "op"), (dict(op=0), "op"), (dict(op="dilate", connectivity=18), "connectivity"),
    (dict(op="dilate", connectivity=True), "connectivity"), (dict(op="dilate", steps=0), "steps"),
    (dict(op="erode", steps=1025), "steps"), (dict(op="open", steps=1.5), "steps"), (dict(op="close", steps=True), "steps"),
    (dict(op="fill_holes", steps=2), "steps"), (dict(op="dilate", band=1), "band"), (dict(op="erode", band=True), "band"),
    (dict(op="fill_holes", band=True), "band"),
])
def test_python_refusals_of_segment_edit(kw, word):
    with pytest.raises(ValueError, match=word):
        renderer_shell().segment_edit(**kw)


def test_python_refusals_of_set_segment_mask():
    r = renderer_shell((16, 16, 24))
    with pytest.raises(ValueError, match="shape"):
        r.set_segment_mask(np.zeros((16, 16, 24), dtype=bool))        # (X, Y, Z) order instead of (Z, Y, X)
    with pytest.raises(ValueError, match="shape"):
        r.set_segment_mask(np.zeros(24 * 16 * 16, dtype=bool))
    with pytest.raises(ValueError, match="bool"):
        r.set_segment_mask(np.zeros((24, 16, 16), dtype=np.uint8))


def test_js_host_carries_the_edit_calls():
    napi = os.path.join(ROOT, "volxel_amd", "napi")
    c = open(os.path.join(napi, "volxel_napi.c")).read()
    js = open(os.path.join(napi, "viewer.js")).read()
    dts = open(os.path.join(napi, "index.d.ts")).read()
    for fn in ("vx_segment_edit(", "vx_segment_write_mask(", "vx_segment_edit_stats("):
        assert fn in c
    for m in ("segmentEdit(", "setSegmentMask(", "segmentEditStats("):
        assert m in js and m in dts
    for op in ER.OPS:
        assert f"'{op}'" in js and f"'{op}'" in dts
