"""The segment store on the GPU (vx_segment_store .. vx_segments_labelmap; DESIGN.md section 2 "Segment store") against the NumPy
restatement (tests/segstore_ref.py, itself pinned to set algebra, the brute-force distance definition and SciPy by
tests/test_segstore_host.py): slots that round-trip bit for bit and do not follow the current segment; every set operation
bit for bit with the mask's statistics; a bone-removal workflow step by step; what the calls invalidate and what they leave;
the overlap counts exact and the directed Hausdorff values and voxels bit for bit under two spacings; the label map in two
list orders; every layout, the masked views, rendering left alone, the C ABI's refusals, device groups and the JS host."""
import ctypes as C
import dataclasses
import json
import math
import shutil

import numpy as np
import pytest

from tests import distance_ref as DR
from tests import islands_ref as IR
from tests import segedit_ref as ER
from tests import segment_ref as SG
from tests import segstore_ref as SS
from tests.common import F32, LAYOUTS, densities, frame, renderer, segment_volumes, upload_volume
from tests.js_host import dump_grid, run_node
from tests.shapes import same_stats, shape_of, uploaded_shapes

SPACINGS = {"unit": (1.0, 1.0, 1.0), "ct": (0.7, 0.7, 1.0)}
VOLUMES = ("noise", "odd", "tube", "phantom")


@pytest.fixture(scope="module")
def volumes():
    v = segment_volumes()
    return {k: v[k] for k in VOLUMES}


_MASKS = {}


def masks(shape):
    """two ragged masks of the shape that overlap partly: the shapes that cross brick faces, edges and corners, and blobs"""
    if shape not in _MASKS:
        m, b = uploaded_shapes(shape), ER.blobs(shape, seed=5, sigma=2.0, q=0.7)
        assert (m & b).any() and (m & ~b).any() and (b & ~m).any()
        for a in (m, b):
            a.setflags(write=False)
        _MASKS[shape] = (m, b)
    return _MASKS[shape]


def pair(shape, kind):
    """(A, B) of a kind"""
    m, b = masks(shape)
    zero, one = np.zeros(shape, dtype=bool), np.ones(shape, dtype=bool)
    return {"overlap": (m, b), "nested": (m & b, m), "equal": (m, m), "disjoint": (m, b & ~m), "empty_a": (zero, m),
            "empty_b": (m, zero), "full_a": (one, m), "full_b": (m, one), "both_empty": (zero, zero)}[kind]


PAIR_KINDS = ("overlap", "nested", "equal", "disjoint", "empty_a", "empty_b", "full_a", "full_b", "both_empty")


def packed_equal(r, want):
    got = r.segment_mask()
    return np.array_equal(SG.packed(got), SG.packed(want))


def same_segment(a, b):
    """two `Segment`s field for field (nan equals nan: the mean of an empty mask)"""
    for f in dataclasses.fields(a):
        x, y = getattr(a, f.name), getattr(b, f.name)
        assert x == y or (isinstance(x, float) and math.isnan(x) and math.isnan(y)), (f.name, x, y)


def refused(fn, *words):
    from volxel_amd import VolxelError
    with pytest.raises(VolxelError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


# ---- the store ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_slots_round_trip_and_do_not_follow_the_current_segment(volumes):
    g = volumes["noise"]
    A, B = masks(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        assert r.stored_segments() == ()
        refused(lambda: r.store_segment(0), "vx_segment_store", "no current segment")
        refused(lambda: r.load_segment(0), "vx_segment_load", "empty")
        r.set_segment_mask(A)
        r.store_segment(0)
        assert r.stored_segments() == (0,) and packed_equal(r, A)          # the current segment is untouched
        r.set_segment_mask(B)
        r.store_segment(31)
        assert r.stored_segments() == (0, 31)
        # the current segment moves on; the slots do not
        r.segment_edit("dilate", steps=2, connectivity=26)
        r.threshold(float(np.quantile(d, 0.8)))
        r.segment_combine("invert")
        assert not packed_equal(r, A) and not packed_equal(r, B)
        for slot, want in ((0, A), (31, B), (0, A)):
            seg = r.load_segment(slot)
            assert packed_equal(r, want)
            same_stats(seg, want, d)
            assert seg.rounds == 0 and seg.brick_visits == 0
            assert r.segment_edit_stats()[0] == 1
        assert r.stored_segments() == (0, 31)                               # a load keeps the slot's copy
        r.segment_edit("erode")                                             # ... and the copy does not follow the loaded mask
        r.load_segment(0)
        assert packed_equal(r, A)
        r.set_segment_mask(B)                                               # storing over an occupied slot replaces it
        r.store_segment(0)
        r.set_segment_mask(A)
        r.load_segment(0)
        assert packed_equal(r, B) and r.stored_segments() == (0, 31)
        r.drop_segment(0)
        assert r.stored_segments() == (31,)
        refused(lambda: r.load_segment(0), "vx_segment_load", "slot 0", "empty")
        assert packed_equal(r, B)                                           # the refused load changed nothing
        r.drop_segment(0)                                                   # dropping an empty slot is fine
        r.drop_segment(17)
        for k in (5, 6, 30):
            r.store_segment(k)
        assert r.stored_segments() == (5, 6, 30, 31)
        r.setup_from_grid(g)                                                # an upload empties the store
        assert r.stored_segments() == ()
        refused(lambda: r.load_segment(31), "empty")
    finally:
        r.close()


# ---- the set operations ---------------------------------------------------------------------------------------------------------
CASES = [(v, k) for v in VOLUMES for k in PAIR_KINDS]


@pytest.mark.gpu
@pytest.mark.parametrize("vol, kind", CASES, ids=[f"{v}-{k}" for v, k in CASES])
def test_every_op_matches_the_restatement(volumes, vol, kind):
    g = volumes[vol]
    A, B = pair(shape_of(g), kind)
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities(vol, g, p)
        r.set_segment_mask(B)
        r.store_segment(3)
        for op in SS.OPS:
            want = SS.combine(op, A, B)
            segs = []
            for _ in range(2):
                r.set_segment_mask(A)
                seg = r.segment_combine(op) if op == "invert" else r.segment_combine(op, 3)
                assert packed_equal(r, want), (vol, kind, op, int(r.segment_mask().sum()), int(want.sum()))
                assert seg.rounds == 0 and seg.brick_visits == 0 and seg.converged
                assert r.segment_edit_stats()[0] == 1
                segs.append(seg)
            same_stats(segs[0], want, d)
            assert segs[0].d_sum == segs[1].d_sum                           # the float64 sum is identical over two runs
            same_segment(segs[0], r.set_segment_mask(want))                 # what the host route reports for the same mask
        r.load_segment(3)
        assert packed_equal(r, B) and r.stored_segments() == (3,)           # no op wrote the slot
        r.segment_combine("xor", 3)                                         # B ^ B
        assert not r.segment_mask().any()
    finally:
        r.close()


@pytest.mark.gpu
def test_bone_removal_workflow_on_the_phantom(volumes):
    from volxel_amd import _checks
    g = volumes["phantom"]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("phantom", g, p)
        sp = _checks.spacing(None, r.volume.grid.transform)
        tissue, bone = SG.predicate(d, 0.40, 0.60), SG.predicate(d, 0.75, np.finfo(np.float32).max)
        assert tissue.any() and bone.any() and not (tissue & bone).any()
        same_stats(r.threshold(0.40, 0.60), tissue, d)
        assert packed_equal(r, tissue)
        r.store_segment(0)
        r.threshold(0.75)
        assert packed_equal(r, bone)
        grown = DR.margin(bone, "grow", 2.0, sp)
        same_stats(r.segment_margin("grow", 2.0), grown, d)
        assert packed_equal(r, grown) and (grown & tissue).any()
        r.store_segment(1)
        same_stats(r.load_segment(0), tissue, d)
        assert packed_equal(r, tissue)
        cut = SS.combine("subtract", tissue, grown)
        same_stats(r.segment_combine("subtract", 1), cut, d)
        assert packed_equal(r, cut) and (cut ^ tissue).any()
        largest, _, n, kept, _ = IR.apply(cut, "keep_largest", 6, keep=1)
        seg = r.keep_largest_islands(1)
        assert packed_equal(r, largest) and (seg.islands, seg.kept) == (n, kept)
        same_stats(seg, largest, d)
        cmp = r.segment_compare(0, hausdorff=False)                         # what the edits removed from the stored tissue
        assert (cmp.count_a, cmp.count_b, cmp.count_and) == SS.counts(largest, tissue) and cmp.count_and == cmp.count_a
    finally:
        r.close()


# ---- what is and is not invalidated ---------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_what_the_calls_invalidate_and_what_they_leave(volumes):
    g = volumes["noise"]
    A, B = masks(shape_of(g))
    one = (1.0, 1.0, 1.0)
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        lo, hi = float(np.quantile(d[d > 0], 0.3)), float(np.quantile(d[d > 0], 0.9))
        pred = SG.predicate(d, lo, hi)
        r.threshold(lo, hi)                                                 # the predicate of band dilation
        r.set_segment_mask(B)
        r.store_segment(1)

        def fresh():
            r.set_segment_mask(A)
            isl = r.islands()
            dist = r.segment_distance(max_distance=4.0, spacing=one)
            return isl, dist, dist.squared()

        for change, want in ((lambda: r.segment_combine("union", 1), A | B), (lambda: r.segment_combine("invert"), ~A),
                             (lambda: r.load_segment(1), B)):
            isl, dist, _ = fresh()
            change()
            assert packed_equal(r, want)
            refused(isl.labels, "no current table")
            refused(lambda: r.island_table(0, 1), "no current table")
            refused(dist.squared, "no current field")
            seg = r.segment_edit("dilate", band=True)                       # the predicate survived
            assert packed_equal(r, ER.edit(want, "dilate", 6, 1, band=pred))
            same_stats(seg, ER.edit(want, "dilate", 6, 1, band=pred), d)
        # what reads, or writes a slot only, keeps the table and the field
        isl, dist, f0 = fresh()
        lab0 = isl.labels()
        r.store_segment(2)
        r.drop_segment(2)
        r.store_segment(4)
        cmp = r.segment_compare(1, hausdorff=False)
        assert (cmp.count_a, cmp.count_b, cmp.count_and) == SS.counts(A, B) and cmp.hausdorff is None and cmp.argmax_ab is None
        r.segments_labelmap([1, 4])
        r.stored_segments()
        assert dist.squared().tobytes() == f0.tobytes() and np.array_equal(isl.labels(), lab0)
        assert packed_equal(r, A)
        # the Hausdorff transforms overwrite the field, and nothing else
        r.segment_compare(1, hausdorff=True, spacing=one)
        refused(dist.squared, "no current field")
        assert np.array_equal(isl.labels(), lab0) and len(r.island_table()) == isl.count
        assert packed_equal(r, A) and r.stored_segments() == (1, 4)
        r.load_segment(1)
        assert packed_equal(r, B)
        r.load_segment(4)
        assert packed_equal(r, A)
    finally:
        r.close()


# ---- the comparison -------------------------------------------------------------------------------------------------------------
_DIRECTED = {}


def ref_directed(vol, sp, A, B):
    """((d2_ab, voxel), (d2_ba, voxel)) of the volume's two masks under a spacing, computed once per session"""
    if (vol, sp) not in _DIRECTED:
        _DIRECTED[vol, sp] = (SS.directed(A, B, SPACINGS[sp]), SS.directed(B, A, SPACINGS[sp]))
    return _DIRECTED[vol, sp]


def check_compare(cmp, A, B, ab, ba):
    a, b, n = SS.counts(A, B)
    assert (cmp.count_a, cmp.count_b, cmp.count_and) == (a, b, n)
    for got, want in ((cmp.dice, SS.dice(a, b, n)), (cmp.jaccard, SS.jaccard(a, b, n))):
        assert got == want or (math.isnan(got) and math.isnan(want))
    for (d2, at, h), (wd2, wat) in (((cmp.d2_ab, cmp.argmax_ab, cmp.hausdorff_ab), ab), ((cmp.d2_ba, cmp.argmax_ba, cmp.hausdorff_ba), ba)):
        assert F32(d2).view(np.uint32) == F32(wd2).view(np.uint32) and at == wat, (d2, at, wd2, wat)
        assert F32(h) == np.sqrt(F32(wd2))
    assert cmp.hausdorff == max(cmp.hausdorff_ab, cmp.hausdorff_ba)


COMPARE_CASES = [(v, s) for v in ("noise", "odd", "tube") for s in sorted(SPACINGS)]


@pytest.mark.gpu
@pytest.mark.parametrize("vol, sp", COMPARE_CASES, ids=[f"{v}-{s}" for v, s in COMPARE_CASES])
def test_comparison_matches_the_restatement_bit_for_bit(volumes, vol, sp):
    g = volumes[vol]
    A, B = masks(shape_of(g))
    ab, ba = ref_directed(vol, sp, A, B)
    assert ab[0] > 0 and ba[0] > 0 and ab != ba
    r = renderer(g, dvr_jitter=False)
    try:
        r.set_segment_mask(B)
        r.store_segment(9)
        r.set_segment_mask(A)
        for _ in range(2):
            check_compare(r.segment_compare(9, spacing=SPACINGS[sp]), A, B, ab, ba)
            st = r.distance_stats()
            assert st[0] == 10 and all(t >= 0 for t in st[1:]) and len(st) == 5
        quick = r.segment_compare(9, hausdorff=False, spacing=SPACINGS[sp])
        assert (quick.count_a, quick.count_b, quick.count_and) == SS.counts(A, B)
        assert quick.dice == SS.dice(*SS.counts(A, B)) and quick.hausdorff_ab is None and quick.d2_ba is None
        assert packed_equal(r, A)
        # the other way round: the directions swap
        r.store_segment(10)
        r.load_segment(9)
        check_compare(r.segment_compare(10, spacing=SPACINGS[sp]), B, A, ba, ab)
    finally:
        r.close()


@pytest.mark.gpu
def test_comparison_of_equal_nested_and_empty_sets(volumes):
    g = volumes["odd"]                  # spacing (1.0, 1.2, 0.9) in its grid transform: what spacing=None stands for
    shape = shape_of(g)
    from volxel_amd import _checks
    r = renderer(g, dvr_jitter=False)
    try:
        sp = _checks.spacing(None, r.volume.grid.transform)
        assert np.allclose(sp, (1.0, 1.2, 0.9), rtol=1e-6)
        for kind in ("equal", "nested", "disjoint", "empty_a", "empty_b", "both_empty", "full_b"):
            A, B = pair(shape, kind)
            r.set_segment_mask(B)
            r.store_segment(0)
            r.set_segment_mask(A)
            cmp = r.segment_compare(0)
            ab, ba = SS.directed(A, B, sp), SS.directed(B, A, sp)
            check_compare(cmp, A, B, ab, ba)
            first = lambda m: tuple(int(q) for q in np.unravel_index(np.flatnonzero(m.ravel())[0], shape)[::-1])
            if kind == "equal":
                assert (cmp.d2_ab, cmp.d2_ba, cmp.hausdorff) == (0.0, 0.0, 0.0) and cmp.dice == 1.0 == cmp.jaccard
                assert cmp.argmax_ab == cmp.argmax_ba == first(A)
            if kind in ("nested", "full_b"):                                # A is a proper subset of B
                assert cmp.d2_ab == 0.0 < cmp.d2_ba and cmp.hausdorff == cmp.hausdorff_ba and cmp.count_and == cmp.count_a
            if kind == "disjoint":
                assert cmp.count_and == 0 and cmp.dice == 0.0 and cmp.d2_ab > 0 and cmp.d2_ba > 0
            if kind == "empty_a":
                assert (cmp.d2_ab, cmp.argmax_ab) == (0.0, (0, 0, 0)) and math.isinf(cmp.d2_ba) and cmp.argmax_ba == first(B)
                assert math.isinf(cmp.hausdorff) and cmp.dice == 0.0
            if kind == "empty_b":
                assert (cmp.d2_ba, cmp.argmax_ba) == (0.0, (0, 0, 0)) and math.isinf(cmp.d2_ab) and cmp.argmax_ab == first(A)
            if kind == "both_empty":
                assert (cmp.d2_ab, cmp.d2_ba, cmp.argmax_ab, cmp.argmax_ba) == (0.0, 0.0, (0, 0, 0), (0, 0, 0))
                assert math.isnan(cmp.dice) and math.isnan(cmp.jaccard) and cmp.hausdorff == 0.0
    finally:
        r.close()


# ---- the label map --------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vol", ("odd", "tube"))
def test_label_map_priority_is_list_order(volumes, vol):
    g = volumes[vol]
    shape = shape_of(g)
    A, B = masks(shape)
    third = ER.blobs(shape, seed=8, sigma=3.0, q=0.5)
    stored = {2: A, 7: B, 31: third, 0: np.zeros(shape, dtype=bool)}
    r = renderer(g, dvr_jitter=False)
    try:
        for slot, m in stored.items():
            r.set_segment_mask(m)
            r.store_segment(slot)
        r.set_segment_mask(B)
        maps = {}
        for order in ((2, 7, 31), (31, 7, 2), (7,), (0, 2), (0,), (31, 0, 7, 2)):
            labels, overlaps = r.segments_labelmap(order)
            want, wover = SS.labelmap([stored[s] for s in order])
            assert labels.dtype == np.uint8 and labels.shape == shape
            assert np.array_equal(labels, want) and overlaps == wover, (vol, order, overlaps, wover)
            maps[order] = labels
        assert not np.array_equal(maps[2, 7, 31], maps[31, 7, 2]) and np.array_equal(maps[2, 7, 31] > 0, maps[31, 7, 2] > 0)
        assert not maps[0,].any()
        if vol == "odd":                                                    # the padding beyond 37 x 29 x 45 is labelled like any voxel
            assert maps[2, 7, 31][45:].any() and maps[2, 7, 31][:, 29:].any() and maps[2, 7, 31][:, :, 37:].any()
        assert packed_equal(r, B)                                           # the current segment is neither read nor changed
        refused(lambda: r.segments_labelmap([2, 5]), "vx_segments_labelmap", "slot 5", "empty")
    finally:
        r.close()


# ---- layouts, views, rendering left alone ---------------------------------------------------------------------------------------
def chain(r, A, B, sp):
    """store, combine, compare and label map in one go: what the layout and device-group tests compare"""
    r.set_segment_mask(B)
    r.store_segment(1)
    r.set_segment_mask(A)
    r.store_segment(0)
    seg = r.segment_combine("subtract", 1)
    mask = r.segment_mask()
    cmp = r.segment_compare(0, spacing=sp)
    labels, overlaps = r.segments_labelmap([1, 0])
    return seg, mask, cmp, labels, overlaps


def check_chain(out, A, B, sp, d):
    seg, mask, cmp, labels, overlaps = out
    cut = SS.combine("subtract", A, B)
    assert np.array_equal(SG.packed(mask), SG.packed(cut))
    same_stats(seg, cut, d)
    check_compare(cmp, cut, A, SS.directed(cut, A, sp), SS.directed(A, cut, sp))
    want, wover = SS.labelmap([B, A])
    assert np.array_equal(labels, want) and overlaps == wover


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout_gives_the_same_chain(volumes, layout):
    """only the statistics read the volume"""
    g = volumes["odd"]
    A, B = masks(shape_of(g))
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        check_chain(chain(r, A, B, SPACINGS["ct"]), A, B, SPACINGS["ct"], densities("odd", g, p))
    finally:
        r.close()


@pytest.mark.gpu
def test_device_group_answers_from_member0(volumes):
    g = volumes["odd"]
    A, B = masks(shape_of(g))
    out = []
    for devices in (None, [0, 0]):
        r = renderer(g, devices=devices, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
            out.append(chain(r, A, B, SPACINGS["ct"]) + (r.stored_segments(),))
        finally:
            r.close()
    check_chain(out[0][:5], A, B, SPACINGS["ct"], densities("odd", g, p))
    (sa, ma, ca, la, oa, ta), (sb, mb, cb, lb, ob, tb) = out
    same_segment(sa, sb)
    assert np.array_equal(ma, mb) and ca == cb and np.array_equal(la, lb) and oa == ob and ta == tb == (0, 1)


MIP = dict(mode="mip", size=(96, 64), dvr_step_voxels=0.5, dvr_jitter=False, max_samples=1 << 20, sample_range=(0.0, 1.0),
           dvr_skip_empty=True, use_env=False, show_environment=False)


@pytest.mark.gpu
def test_a_combine_under_a_view_restarts_and_shows_the_new_mask(volumes):
    g = volumes["noise"]
    A, B = masks(shape_of(g))
    r = renderer(g, layout=LAYOUTS["brickf32"], **MIP)
    fresh = renderer(g, layout=LAYOUTS["brickf32"], **MIP)
    try:
        r.set_segment_mask(B)
        r.store_segment(0)
        r.set_segment_mask(A)
        r.segment_view = "hide"
        before = frame(r)[0].copy()
        r.render(frames=2, in_flight=1)
        assert r.frame_index == 3
        r.segment_combine("union", 0)
        assert r.frame_index == 0                       # the host restarted accumulation: the picture changed
        img = frame(r)[0]
        fresh.set_segment_mask(A | B)
        fresh.segment_view = "hide"
        want = frame(fresh)[0]
        assert np.array_equal(img.view(np.uint32), want.view(np.uint32)) and not np.array_equal(img, before)
        r.render(frames=1, in_flight=1)
        r.load_segment(0)                               # a load shows a new mask too
        assert r.frame_index == 0
        fresh.set_segment_mask(B)
        assert np.array_equal(frame(r)[0].view(np.uint32), frame(fresh)[0].view(np.uint32))
        r.render(frames=1, in_flight=1)
        n = r.frame_index
        r.store_segment(5)                              # what leaves the mask alone does not restart
        r.segment_compare(0)
        r.segments_labelmap([0, 5])
        r.drop_segment(5)
        assert r.frame_index == n
    finally:
        r.close()
        fresh.close()


@pytest.mark.gpu
def test_rendering_is_left_alone_with_the_view_off(volumes):
    g = volumes["noise"]
    r = renderer(g, dvr_jitter=False)
    try:
        r.bind_uniforms()
        r.segment((10, 10, 10), 0.2, connectivity=26)
        r.reset_counters()
        r.restart_rendering()
        r.render(frames=2, in_flight=1)
        a = r.read_accum().copy()
        c1 = r.counters()
        c1 = {f: getattr(c1, f) for f, _ in c1._fields_}
        st = r.segment_stats()
        r.store_segment(0)
        r.segment_edit("dilate")
        r.store_segment(1)
        for op in SS.OPS[:4]:
            r.segment_combine(op, 0)
            r.load_segment(1)
        r.segment_combine("invert")
        r.segment_compare(0, hausdorff=False)
        r.segment_compare(1)
        r.segments_labelmap([1, 0])
        r.stored_segments()
        r.drop_segment(1)
        b = r.read_accum().copy()
        c2 = r.counters()
        c2 = {f: getattr(c2, f) for f, _ in c2._fields_}
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert c1 == c2 and r.frame_index == 2
        assert r.segment_stats() == st
        r.render(frames=1, in_flight=1)           # accumulation goes on where it was
        assert r.counters().frames == c1["frames"] + 1 and r.frame_index == 3
    finally:
        r.close()


# ---- the C ABI ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_refusals_name_the_field_and_change_nothing(volumes):
    from volxel_amd import _abi
    g = volumes["noise"]
    lib = _abi.load_library()
    n = 64 ** 3
    A, B = masks((64, 64, 64))
    pa, pb = SG.packed(A), SG.packed(B)
    back = np.zeros(n // 8, dtype=np.uint8)
    labels = np.zeros(n, dtype=np.uint8)
    seg, res = _abi.VxSegmentResult(), _abi.VxCompareResult()
    cq, pq = _abi.VxCombineParams(), _abi.VxCompareParams()
    cq.op, cq.slot = 0, 0
    pq.slot, pq.hausdorff = 0, 1
    pq.spacing[:] = (1.0, 1.0, 1.0)
    occ, over = C.c_uint32(77), C.c_uint64()
    u32s = lambda *v: (C.c_uint32 * len(v))(*v)
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        err = lambda: lib.vx_last_error(ctx)
        calls = {
            "store": lambda: lib.vx_segment_store(ctx, 0), "load": lambda: lib.vx_segment_load(ctx, 0, C.byref(seg)),
            "drop": lambda: lib.vx_segment_drop(ctx, 0), "slots": lambda: lib.vx_segment_slots(ctx, C.byref(occ)),
            "combine": lambda: lib.vx_segment_combine(ctx, C.byref(cq), C.byref(seg)),
            "compare": lambda: lib.vx_segment_compare(ctx, C.byref(pq), C.byref(res)),
            "labelmap": lambda: lib.vx_segments_labelmap(ctx, u32s(0), 1, labels.ctypes.data, n, C.byref(over))}
        for name, call in calls.items():
            assert call() == 3 and b"no volume" in err(), name                                           # VX_ERR_NO_VOLUME
        assert upload_volume(lib, ctx, g) == 0
        for name, call in calls.items():
            assert call() == 1 and b"vx_set_params" in err(), name
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_resize(ctx, 64, 48) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        assert lib.vx_segment_slots(ctx, C.byref(occ)) == 0 and occ.value == 0
        for name in ("store", "combine", "compare"):
            assert calls[name]() == 1 and b"no current segment" in err(), name
        cq.op = 4
        assert calls["combine"]() == 1 and b"no current segment" in err()                                # INVERT needs one too
        cq.op = 0
        for name in ("load", "labelmap"):
            assert calls[name]() == 1 and b"empty" in err(), name
        assert lib.vx_segment_write_mask(ctx, pb.ctypes.data, n // 8, None) == 0
        assert calls["compare"]() == 1 and b"empty" in err()
        assert calls["store"]() == 0 and lib.vx_segment_store(ctx, 31) == 0
        assert lib.vx_segment_write_mask(ctx, pa.ctypes.data, n // 8, None) == 0
        assert lib.vx_segment_drop(ctx, 12) == 0                                                         # an empty slot: VX_OK

        def unchanged(what):
            assert lib.vx_segment_read_mask(ctx, back.ctypes.data, n // 8) == 0 and np.array_equal(back, pa), what
            assert lib.vx_segment_slots(ctx, C.byref(occ)) == 0 and occ.value == (1 | 1 << 31), what

        def refuse(rc, *words):
            assert rc == 1, (words, err())
            for w in words:
                assert w in err(), (w, err())
            unchanged(words)

        unchanged("start")
        for bad in (32, 33, 0xffffffff):                                                                 # a slot that does not exist
            refuse(lib.vx_segment_store(ctx, bad), b"vx_segment_store", b"slot")
            refuse(lib.vx_segment_load(ctx, bad, C.byref(seg)), b"vx_segment_load", b"slot")
            refuse(lib.vx_segment_drop(ctx, bad), b"vx_segment_drop", b"slot")
            cq.slot = pq.slot = bad
            refuse(lib.vx_segment_combine(ctx, C.byref(cq), None), b"vx_segment_combine", b"slot")
            refuse(lib.vx_segment_compare(ctx, C.byref(pq), None), b"vx_segment_compare", b"slot")
            refuse(lib.vx_segments_labelmap(ctx, u32s(0, bad), 2, labels.ctypes.data, n, None), b"vx_segments_labelmap", b"slot")
        cq.slot = pq.slot = 5                                                                            # an empty one
        refuse(lib.vx_segment_load(ctx, 5, None), b"vx_segment_load", b"empty")
        refuse(lib.vx_segment_combine(ctx, C.byref(cq), None), b"vx_segment_combine", b"empty")
        refuse(lib.vx_segment_compare(ctx, C.byref(pq), None), b"vx_segment_compare", b"empty")
        refuse(lib.vx_segments_labelmap(ctx, u32s(0, 5), 2, labels.ctypes.data, n, None), b"vx_segments_labelmap", b"empty")
        cq.slot = pq.slot = 0
        for bad in (-1, 5, 100):
            cq.op = bad
            refuse(lib.vx_segment_combine(ctx, C.byref(cq), None), b"op")
        cq.op = 0
        for bad in (-1, 2):
            pq.hausdorff = bad
            refuse(lib.vx_segment_compare(ctx, C.byref(pq), None), b"hausdorff")
        pq.hausdorff = 1
        for a in range(3):
            for bad in (0.0, -1.0, float("nan"), float("inf")):
                sp = [1.0, 1.0, 1.0]
                sp[a] = bad
                pq.spacing[:] = sp
                refuse(lib.vx_segment_compare(ctx, C.byref(pq), None), b"spacing[%d]" % a)
        pq.hausdorff = 0                                                                                 # the spacing is not read
        assert lib.vx_segment_compare(ctx, C.byref(pq), C.byref(res)) == 0
        assert (res.count_a, res.count_b, res.count_and) == SS.counts(A, B) and res.d2_ab == 0.0 and tuple(res.argmax_ba) == (0, 0, 0)
        pq.spacing[:] = (1.0, 1.0, 1.0)
        refuse(lib.vx_segment_combine(ctx, None, None), b"params")
        refuse(lib.vx_segment_compare(ctx, None, None), b"params")
        refuse(lib.vx_segment_slots(ctx, None), b"occupied")
        refuse(lib.vx_segments_labelmap(ctx, None, 1, labels.ctypes.data, n, None), b"slots")
        refuse(lib.vx_segments_labelmap(ctx, u32s(0), 1, None, n, None), b"labels")
        for wrong in (n - 1, n + 1, 0, n // 8):
            refuse(lib.vx_segments_labelmap(ctx, u32s(0), 1, labels.ctypes.data, wrong, None), b"nvoxels")
        refuse(lib.vx_segments_labelmap(ctx, u32s(0, 31, 0), 3, labels.ctypes.data, n, None), b"duplicate")
        refuse(lib.vx_segments_labelmap(ctx, u32s(0), 0, labels.ctypes.data, n, None), b"n = 0")
        refuse(lib.vx_segments_labelmap(ctx, u32s(*([0] * 33)), 33, labels.ctypes.data, n, None), b"n = 33")
        # what is legal: NULL outs, INVERT with any slot value, overlaps NULL
        assert lib.vx_segments_labelmap(ctx, u32s(31, 0), 2, labels.ctypes.data, n, None) == 0
        assert np.array_equal(labels.reshape(A.shape), SS.labelmap([B, B])[0])
        assert lib.vx_segment_compare(ctx, C.byref(pq), None) == 0 and lib.vx_segment_load(ctx, 31, None) == 0
        cq.op, cq.slot = 4, 1000
        assert lib.vx_segment_combine(ctx, C.byref(cq), None) == 0
        assert lib.vx_segment_read_mask(ctx, back.ctypes.data, n // 8) == 0 and np.array_equal(back, SG.packed(~B))
        launches = C.c_uint32()
        assert lib.vx_segment_edit_stats(ctx, C.byref(launches), None) == 0 and launches.value == 1
        assert upload_volume(lib, ctx, g) == 0                                                           # an upload empties the store
        assert lib.vx_segment_slots(ctx, C.byref(occ)) == 0 and occ.value == 0
        assert lib.vx_segment_load(ctx, 0, None) == 1 and b"empty" in err()
        assert lib.vx_segment_store(ctx, 0) == 1 and b"no current segment" in err()
        assert lib.vx_segment_write_mask(ctx, pa.ctypes.data, n // 8, None) == 0                         # ... and storing works again
        assert lib.vx_segment_store(ctx, 4) == 0 and lib.vx_segment_slots(ctx, C.byref(occ)) == 0 and occ.value == 1 << 4
        assert lib.vx_segment_load(ctx, 4, C.byref(seg)) == 0 and seg.count == int(A.sum())
    finally:
        lib.vx_destroy(ctx)


# ---- the JS host ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_has_the_python_bytes(volumes, tmp_path):
    g = volumes["odd"]
    A, B = masks(shape_of(g))
    s = SPACINGS["ct"]
    r = renderer(g, dvr_jitter=False)
    try:
        seg, mask, cmp, labels, overlaps = chain(r, A, B, s)
        quick = r.segment_compare(1, hausdorff=False)
        loaded = r.load_segment(1)
        stored = r.stored_segments()
    finally:
        r.close()
    dump_grid(tmp_path, g)
    SG.packed(A).tofile(tmp_path / "a.bin")
    SG.packed(B).tofile(tmp_path / "b.bin")
    (tmp_path / "args.json").write_text(json.dumps({"spacing": list(s)}))
    body = r"""
const a = JSON.parse(fs.readFileSync(path.join(dir, 'args.json')));
const before = r.storedSegments();
r.setSegmentMask(rd('b.bin', Uint8Array));
r.storeSegment(1);
r.setSegmentMask(rd('a.bin', Uint8Array));
r.storeSegment(0);
const seg = r.segmentCombine('subtract', 1);
save('mask.bin', r.segmentMask());
const cmp = r.segmentCompare(0, { spacing: a.spacing });
const map = r.segmentsLabelmap([1, 0]);
save('labels.bin', map.labels);
const quick = r.segmentCompare(1, { hausdorff: false });
const loaded = r.loadSegment(1);
save('loaded.bin', r.segmentMask());
const stored = r.storedSegments();
const msg = (f) => { try { f(); return ''; } catch (e) { return String(e.message); } };
const refusals = [msg(() => r.segmentCombine('invert', 0)), msg(() => r.segmentCombine('union')), msg(() => r.storeSegment(32)),
  msg(() => r.segmentsLabelmap([0, 0])), msg(() => r.segmentsLabelmap([])), msg(() => r.segmentCombine('nand', 0))];
r.dropSegment(0);
refusals.push(msg(() => r.loadSegment(0)));
console.log(JSON.stringify({ before, seg, cmp, overlaps: map.overlaps, quick, loaded, stored, after: r.storedSegments(), refusals,
  st: r.distanceStats() }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert np.array_equal(np.fromfile(tmp_path / "mask.bin", dtype=np.uint8), SG.packed(mask))
    assert np.fromfile(tmp_path / "labels.bin", dtype=np.uint8).tobytes() == labels.tobytes() and out["overlaps"] == overlaps
    assert np.array_equal(np.fromfile(tmp_path / "loaded.bin", dtype=np.uint8), SG.packed(B))
    for js, py in ((out["seg"], seg), (out["loaded"], loaded)):
        assert js["count"] == py.count and tuple(js["bboxLo"]) == py.bbox_lo and tuple(js["bboxHi"]) == py.bbox_hi
        assert js["dSum"] == py.d_sum and js["converged"] is True and js["rounds"] == 0
    js = out["cmp"]
    assert (js["countA"], js["countB"], js["countAnd"]) == (cmp.count_a, cmp.count_b, cmp.count_and)
    assert js["dice"] == cmp.dice and js["jaccard"] == cmp.jaccard
    assert F32(js["d2Ab"]) == F32(cmp.d2_ab) and F32(js["d2Ba"]) == F32(cmp.d2_ba)
    assert F32(js["hausdorffAb"]) == F32(cmp.hausdorff_ab) and F32(js["hausdorffBa"]) == F32(cmp.hausdorff_ba)
    assert F32(js["hausdorff"]) == F32(cmp.hausdorff)
    assert tuple(js["argmaxAb"]) == cmp.argmax_ab and tuple(js["argmaxBa"]) == cmp.argmax_ba
    q = out["quick"]
    assert (q["countA"], q["countB"], q["countAnd"]) == (quick.count_a, quick.count_b, quick.count_and) and q["dice"] == quick.dice
    assert q["hausdorff"] is None and q["d2Ab"] is None and q["argmaxBa"] is None
    assert out["before"] == [] and tuple(out["stored"]) == stored == (0, 1) and out["after"] == [1]
    assert out["st"]["launches"] == 10
    for text, word in zip(out["refusals"], ("slot", "slot", "slot", "slots", "slots", "op", "empty")):
        assert word in text, (word, text)
