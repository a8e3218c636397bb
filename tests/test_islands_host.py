"""The islands restatement (tests/islands_ref.py) on the CPU: the SciPy and the NumPy restatement agree; closed forms (separated
cubes, equal cubes ordered by anchor, diagonal chains, the checkerboard brick); the laws the ops obey; negative controls -- a
reference with the tie rule reversed, with 18-connectivity, with anchors in brick-major order must each fail a case, so the
cases are known to tell these apart; and the host surface (header, bindings, argument checks that need no GPU)."""
import ctypes as C

import numpy as np
import pytest

from tests import islands_ref as IR
from tests import segment_ref as SG

CONNS = (6, 26)


def _cubes(shape, cubes):
    m = np.zeros(shape, dtype=bool)
    for (x, y, z), s in cubes:
        m[z:z + s, y:y + s, x:x + s] = True
    return m


def _noise(shape, p, seed):
    return np.random.default_rng(seed).random(shape) < p


def _checkerboard(shape=(16, 16, 16), at=(8, 0, 8)):
    m = np.zeros(shape, dtype=bool)
    z, y, x = np.indices((8, 8, 8))
    m[at[2]:at[2] + 8, at[1]:at[1] + 8, at[0]:at[0] + 8] = (x + y + z) % 2 == 0
    return m


@pytest.mark.parametrize("conn", CONNS)
@pytest.mark.parametrize("p", [0.03, 0.08, 0.2])
def test_scipy_and_numpy_restatements_agree(conn, p):
    m = _noise((12, 16, 24), p, seed=int(p * 100) + conn)
    a, b = IR.scipy_islands(m, conn), IR.numpy_islands(m, conn)
    assert len(a) > 3 and IR.same(a, b)
    assert int(a.counts.sum()) == int(m.sum()) and np.array_equal(a.labels != 0, m)
    assert np.all(np.diff(a.counts.astype(np.int64)) <= 0)                 # count descending


@pytest.mark.parametrize("conn", CONNS)
def test_separated_cubes_give_their_counts_anchors_and_boxes_in_order(conn):
    cubes = [((20, 3, 2), 2), ((1, 1, 1), 5), ((10, 10, 10), 3), ((26, 20, 9), 1), ((2, 20, 22), 4)]
    t = IR.islands(_cubes((32, 32, 32), cubes), conn)
    by_size = sorted(cubes, key=lambda c: -c[1])
    assert t.rows() == [(s ** 3, a, a, tuple(v + s - 1 for v in a)) for a, s in by_size]
    assert IR.same(t, IR.numpy_islands(_cubes((32, 32, 32), cubes), conn))


@pytest.mark.parametrize("conn", CONNS)
def test_equal_cubes_are_ordered_by_anchor_in_c_order(conn):
    # C order is (z, y, x): the cube lower in z comes first although its x is larger
    cubes = [((2, 9, 12), 3), ((20, 2, 4), 3), ((9, 1, 4), 3), ((9, 20, 3), 3)]
    t = IR.islands(_cubes((24, 24, 24), cubes), conn)
    assert [a for _, a, _, _ in t.rows()] == [(9, 20, 3), (9, 1, 4), (20, 2, 4), (2, 9, 12)]
    assert list(t.counts) == [27] * 4
    assert [int(t.labels[a[2], a[1], a[0]]) for a in t.anchors] == [1, 2, 3, 4]


def test_a_diagonal_chain_is_one_island_under_26_and_voxels_under_6():
    m = np.zeros((24, 24, 24), dtype=bool)
    pts = [(k, 23 - k, k) for k in range(24)]
    for x, y, z in pts:
        m[z, y, x] = True
    t26, t6 = IR.islands(m, 26), IR.islands(m, 6)
    assert t26.rows() == [(24, (0, 23, 0), (0, 0, 0), (23, 23, 23))]
    assert len(t6) == 24 and list(t6.counts) == [1] * 24 and t6.anchors == pts      # ties: anchors ascending in z
    assert IR.same(t6, IR.numpy_islands(m, 6))


def test_the_checkerboard_brick_is_256_islands_under_6_and_one_under_26():
    m = _checkerboard()
    t6, t26 = IR.islands(m, 6), IR.islands(m, 26)
    assert len(t6) == 256 and int(t6.counts.max()) == 1
    assert len(t26) == 1 and int(t26.counts[0]) == 256


@pytest.mark.parametrize("conn", CONNS)
def test_laws_of_the_ops(conn):
    m = _noise((16, 24, 24), 0.22, seed=9)
    t = IR.islands(m, conn)
    n = len(t)
    assert n > 5
    for op, kw in (("keep_largest", dict(keep=n)), ("keep_largest", dict(keep=n + 7)), ("remove_small", dict(min_voxels=1)),
                   ("label", {})):
        nm, nt, before, kept, largest = IR.apply(m, op, conn, **kw)
        assert np.array_equal(nm, m) and IR.same(nt, t) and (before, kept, largest) == (n, n, int(t.counts[0]))
    # KEEP_LARGEST(1) = KEEP_AT(anchor of island 0) = the component of that anchor
    a = IR.apply(m, "keep_largest", conn, keep=1)[0]
    b = IR.apply(m, "keep_at", conn, seed=t.anchors[0])[0]
    assert np.array_equal(a, b) and np.array_equal(a, SG.component(m, t.anchors[0], conn)) and int(a.sum()) == int(t.counts[0])
    # KEEP_AT outside the mask: the empty set
    z, y, x = (int(v[0]) for v in np.nonzero(~m))
    e = IR.apply(m, "keep_at", conn, seed=(x, y, z))
    assert not e[0].any() and e[3] == 0 and len(e[1]) == 0
    # the kept masks partition M
    acc = np.zeros_like(m, dtype=np.int32)
    for k in range(n):
        acc += IR.apply(m, "keep_at", conn, seed=t.anchors[k], table=t)[0]
    assert np.array_equal(acc, m.astype(np.int32))
    # REMOVE_SMALL is monotone in min_voxels, and its table is the table of its mask
    prev = m
    for mv in (1, 2, 3, 5, 9, 10 ** 6):
        nm, nt, _, kept, _ = IR.apply(m, "remove_small", conn, min_voxels=mv)
        assert not (nm & ~prev).any() and kept == int((t.counts >= mv).sum())
        assert IR.same(nt, IR.islands(nm, conn))
        prev = nm
    assert not prev.any()
    # KEEP_LARGEST(k): the filtered table is the table of the new mask
    for k in (1, 2, 4):
        nm, nt, _, kept, _ = IR.apply(m, "keep_largest", conn, keep=k)
        assert kept == k and IR.same(nt, IR.islands(nm, conn))


def test_an_empty_mask_has_no_islands():
    m = np.zeros((8, 8, 16), dtype=bool)
    for conn in CONNS:
        t = IR.islands(m, conn)
        assert len(t) == 0 and not t.labels.any() and IR.same(t, IR.numpy_islands(m, conn))
        for op, kw in (("keep_largest", dict(keep=1)), ("remove_small", dict(min_voxels=1)), ("keep_at", dict(seed=(0, 0, 0)))):
            nm, nt, before, kept, largest = IR.apply(m, op, conn, **kw)
            assert not nm.any() and (before, kept, largest) == (0, 0, 0)


def test_negative_controls_fail_a_case():
    """each wrong reference differs from the restatement on one of the cases above"""
    equal = _cubes((24, 24, 24), [((2, 9, 12), 3), ((20, 2, 4), 3), ((9, 1, 4), 3), ((9, 20, 3), 3)])
    assert not IR.same(IR.reversed_ties(equal, 6), IR.islands(equal, 6))
    m = np.zeros((24, 24, 24), dtype=bool)
    for k in range(24):
        m[k, 23 - k, k] = True                     # corner links only: 18-connectivity does not follow them
    assert len(IR.conn18(m)) == 24 and len(IR.islands(m, 26)) == 1
    e = np.zeros((16, 16, 16), dtype=bool)
    for k in range(16):
        e[4, k, k] = True                          # edge links: 18 follows them, 6 does not
    assert len(IR.conn18(e)) == 1 and len(IR.islands(e, 6)) == 16
    # an L that starts in brick x = 1 and reaches brick x = 0 one row later: first in C order (9, 0, 0), in brick-major (7, 1, 0)
    L = np.zeros((8, 8, 16), dtype=bool)
    L[0, 0, 9] = L[0, 1, 9] = L[0, 1, 8] = L[0, 1, 7] = True
    assert IR.islands(L, 6).anchors == [(9, 0, 0)] and IR.brick_major_anchors(L, 6).anchors == [(7, 1, 0)]
    assert not IR.same(IR.brick_major_anchors(L, 6), IR.islands(L, 6))
    # and the controls agree with the restatement where their fault does not show
    one = _cubes((16, 16, 16), [((1, 1, 1), 4), ((9, 9, 9), 2)])
    assert IR.same(IR.reversed_ties(one, 6), IR.islands(one, 6)) and IR.same(IR.brick_major_anchors(one, 6), IR.islands(one, 6))


def test_thresholded_noise_has_the_islands_the_gpu_cases_count_on():
    """small_noise(64) at its 0.9 quantile: 91 islands under 6 and 68 under 26, with ties of size 1 and 2"""
    from tests.common import small_noise
    v, _ = small_noise(64)
    d = v.astype(np.float32)
    m = d >= np.quantile(d, 0.9)
    t6, t26 = IR.islands(m, 6), IR.islands(m, 26)
    assert int((t6.counts == 1).sum()) > 1 and int((t6.counts == 2).sum()) > 1
    assert len(t6) > len(t26) > 10


# ---- the host surface ---------------------------------------------------------------------------------------------------------
NAMES = ("vx_segment_threshold", "vx_segment_islands", "vx_islands_read", "vx_islands_read_labels", "vx_islands_stats")


def test_header_declares_the_entry_points_and_the_library_exports_them(native_lib):
    from volxel_amd import _abi
    for name in NAMES:
        assert name in _abi.declared_symbols("volxel_hip.h")
        assert getattr(native_lib, name) is not None


def test_struct_layouts():
    from volxel_amd import _abi
    assert C.sizeof(_abi.VxIslandsParams) == 40 and _abi.VxIslandsParams.keep.offset == 8 and _abi.VxIslandsParams.seed.offset == 24
    assert C.sizeof(_abi.VxSegmentResult) == 64
    assert C.sizeof(_abi.VxIslandsResult) == 24 + 64 and _abi.VxIslandsResult.seg.offset == 24
    assert C.sizeof(_abi.VxIsland) == 48 and _abi.VxIsland.label.offset == 44
    assert _abi.ISLANDS_OPS == {"label": 0, "keep_largest": 1, "remove_small": 2, "keep_at": 3}


def test_island_segment_keeps_the_fields_of_segment():
    from volxel_amd.renderer import IslandSegment, Segment
    names = list(Segment.__dataclass_fields__)
    assert list(IslandSegment.__dataclass_fields__)[:len(names)] == names
    assert list(IslandSegment.__dataclass_fields__)[len(names):] == ["islands", "kept", "largest"]
    assert issubclass(IslandSegment, Segment)


def test_the_node_host_declares_the_calls():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    dts = open(os.path.join(root, "volxel_amd", "napi", "index.d.ts")).read()
    js = open(os.path.join(root, "volxel_amd", "napi", "viewer.js")).read()
    for name in ("threshold", "islands", "keepLargestIslands", "removeSmallIslands", "keepIslandAt", "islandsStats"):
        assert f"  {name}(" in dts and f"  {name}(" in js, name
