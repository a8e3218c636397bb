"""The histograms on the GPU (vx_histogram; DESIGN.md section 2 "Histograms") against the NumPy restatement
(tests/histogram_ref.py, itself pinned to np.histogram, np.sort and a brute-force Otsu by tests/test_histogram_host.py): counts,
below, above, count and the extremes bit for bit, the float64 sums within the bound the segment's own sum is held to; inputs
that pile most voxels into one bin; boxes that cut bricks; the segment and a slot as the region; the raw key passes, the order
statistics and the percentiles bitwise against np.sort; every layout; that the calls change nothing; Otsu; the C ABI's refusals;
device groups and the JS host."""
import ctypes as C
import json
import math
import shutil
import struct

import numpy as np
import pytest

from tests import histogram_ref as HR
from tests import segment_ref as SG
from tests.common import F32, LAYOUTS, densities, frame, renderer, segment_volumes, upload_volume
from tests.js_host import dump_grid, run_node
from tests.shapes import shape_of, uploaded_shapes

VOLUMES = ("noise", "odd", "phantom")
CUT_BOX = ((3, 0, 5), (60, 50, 63))                 # cuts bricks off the multiples of 8
BOXES = {"voxel": ((13, 22, 37), (13, 22, 37)), "brick": ((8, 16, 24), (15, 23, 31)), "cut": CUT_BOX,
         "inner": ((17, 9, 25), (44, 30, 41))}      # inner: whole bricks lie outside it on every axis


@pytest.fixture(scope="module")
def volumes():
    v = segment_volumes()
    return {k: v[k] for k in VOLUMES}


_MASKS, _REF = {}, {}


def ragged(shape):
    if shape not in _MASKS:
        m = uploaded_shapes(shape)
        m.setflags(write=False)
        _MASKS[shape] = m
    return _MASKS[shape]


def in_box(shape, box):
    m = np.zeros(shape, dtype=bool)
    if box is None:
        m[:] = True
    else:
        (x0, y0, z0), (x1, y1, z1) = box
        m[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
    return m


def region(d, mask=None, box=None):
    """the densities of R, flat"""
    sel = in_box(d.shape, box)
    if mask is not None:
        sel &= mask
    return d[sel]


def ref_moments(key, dr):
    """HR.moments of a region, once per session for the regions several tests share (key None: not kept)"""
    if key is None:
        return HR.moments(dr)
    if key not in _REF:
        _REF[key] = HR.moments(dr)
    return _REF[key]


def same_histogram(h, dr, bins, lo, hi, key=None):
    """a `Histogram` against the restatement on the region's densities"""
    counts, below, above = HR.linear(dr, bins, lo, hi)
    m = ref_moments(key, dr)
    assert h.counts.dtype == np.uint64 and np.array_equal(h.counts, counts), np.flatnonzero(h.counts != counts)[:8]
    assert (h.below, h.above, h.count) == (below, above, m["count"]) and below + above + int(counts.sum()) == h.count
    assert F32(h.d_min).view(np.uint32) == F32(m["d_min"]).view(np.uint32) and F32(h.d_max).view(np.uint32) == F32(m["d_max"]).view(np.uint32)
    for got, want in ((h.d_sum, m["d_sum"]), (h.d_sum2, m["d_sum2"])):
        print(f"sum {got!r} against {want!r}")
        assert abs(got - want) <= 1e-9 * abs(want), (got, want)
    assert np.array_equal(h.edges, HR.edges(bins, lo, hi))
    mean, std = HR.mean_std(dict(m, d_sum=h.d_sum, d_sum2=h.d_sum2))
    assert (h.mean == mean and h.std == std) or (m["count"] == 0 and math.isnan(h.mean) and math.isnan(h.std))


def as_bytes(h):
    return h.counts.tobytes() + struct.pack("<3Q2d2f", h.count, h.below, h.above, h.d_sum, h.d_sum2, h.d_min, h.d_max)


def refused(fn, *words):
    from volxel_amd import VolxelError
    with pytest.raises(VolxelError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def key_call(r, source, prefix, p, b, box=None, moments=0):
    """one raw VX_HIST_KEY pass through the Python host's own call"""
    q = r._histogram_params("histogram", source, box)
    q.rule, q.prefix, q.prefix_bits, q.key_bits, q.moments = 1, prefix, p, b, moments
    r.bind_uniforms()
    return r._histogram_call(q, 1 << b)


# ---- the whole volume -----------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vol", VOLUMES)
def test_volume_histograms_match_the_restatement(volumes, vol):
    g = volumes[vol]
    r = renderer(g, dvr_jitter=False)
    try:
        assert r.histogram_stats() == (0, 0.0, 0.0)
        p = r.bind_uniforms()
        d = densities(vol, g, p)
        dr = d.ravel()
        for bins in (1, 7, 256, 4096):
            h = r.histogram(bins=bins)
            same_histogram(h, dr, bins, 0.0, 1.0, key=(vol, "all"))
            assert h.below == 0 and h.above == 0
        pos = dr[dr > 0]
        lo, hi = float(np.quantile(pos, 0.3)), float(np.quantile(pos, 0.8))
        h = r.histogram(bins=100, range=(lo, hi))
        same_histogram(h, dr, 100, lo, hi, key=(vol, "all"))
        assert h.below > 0 and h.above > 0
        again = r.histogram(bins=100, range=(lo, hi))
        assert as_bytes(h) == as_bytes(again)                       # the sums included: a fixed order of addition
        launches, hist_ms, mom_ms = r.histogram_stats()
        assert launches == 2 and hist_ms > 0.0 and mom_ms > 0.0
    finally:
        r.close()


@pytest.mark.gpu
def test_contention_on_one_bin_loses_and_doubles_nothing(volumes):
    """the smallest inputs on which a lost or doubled LDS update shows: half of `noise` is exactly 0 and three quarters of
    `phantom` are air, so one bin of 4096 takes most updates of most waves; with one bin every update goes to one address"""
    for vol, share in (("noise", 0.5), ("phantom", 0.7)):
        g = volumes[vol]
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
            dr = densities(vol, g, p).ravel()
            want, _, _ = HR.linear(dr, 4096, 0.0, 1.0)
            assert int(want.max()) >= share * dr.size
            for bins in (4096, 1024, 1025, 1):                      # 1024 / 1025: per-wave copies and one copy per workgroup
                same_histogram(r.histogram(bins=bins), dr, bins, 0.0, 1.0, key=(vol, "all"))
            assert int(r.histogram(bins=1).counts[0]) == dr.size
        finally:
            r.close()


# ---- boxes ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vol", ("noise", "odd"))
def test_boxes_cut_bricks_and_skip_bricks(volumes, vol):
    g = volumes[vol]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities(vol, g, p)
        assert d.shape == (64, 64, 64)
        for name, box in BOXES.items():
            dr = region(d, box=box)
            h = r.histogram(bins=64, box=box)
            same_histogram(h, dr, 64, 0.0, 1.0)
            (x0, y0, z0), (x1, y1, z1) = box
            assert h.count == (x1 - x0 + 1) * (y1 - y0 + 1) * (z1 - z0 + 1), name
        one = r.histogram(bins=16, box=BOXES["voxel"])
        x, y, z = BOXES["voxel"][0]
        assert one.count == 1 and F32(one.d_min) == F32(one.d_max) == d[z, y, x] and one.d_sum == float(d[z, y, x])
        whole = ((0, 0, 0), (63, 63, 63))
        assert as_bytes(r.histogram(bins=64, box=whole)) == as_bytes(r.histogram(bins=64))
    finally:
        r.close()


# ---- the segment and the slots ------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("vol", ("noise", "odd"))
def test_segment_source_reads_the_current_mask(volumes, vol):
    g = volumes[vol]
    M = ragged(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities(vol, g, p)
        refused(lambda: r.histogram(source="segment"), "vx_histogram", "no current segment")
        seg = r.set_segment_mask(M)
        h = r.histogram(bins=256, source="segment")
        same_histogram(h, region(d, M), 256, 0.0, 1.0)
        # the segment's own statistics: the same voxels added in the same order
        assert (h.count, F32(h.d_min), F32(h.d_max), h.d_sum) == (seg.count, F32(seg.d_min), F32(seg.d_max), seg.d_sum)
        same_histogram(r.histogram(bins=33, source="segment", box=CUT_BOX), region(d, M, CUT_BOX), 33, 0.0, 1.0)
        seg = r.segment_edit("dilate", steps=2, connectivity=26)              # the new mask is read
        h2 = r.histogram(bins=256, source="segment")
        same_histogram(h2, region(d, r.segment_mask()), 256, 0.0, 1.0)
        assert h2.count == seg.count > h.count and h2.d_sum == seg.d_sum
        r.set_segment_mask(np.zeros_like(M))                                  # the empty mask: everything is 0
        e = r.histogram(bins=8, source="segment")
        assert not e.counts.any() and (e.count, e.below, e.above, e.d_sum, e.d_sum2, e.d_min, e.d_max) == (0, 0, 0, 0.0, 0.0, 0.0, 0.0)
        assert math.isnan(e.mean) and math.isnan(e.std)
        r.set_segment_mask(np.ones_like(M))                                   # the full mask: the VOLUME result field for field
        assert as_bytes(r.histogram(bins=300, source="segment")) == as_bytes(r.histogram(bins=300))
        assert as_bytes(r.histogram(bins=300, source="segment", box=CUT_BOX)) == as_bytes(r.histogram(bins=300, box=CUT_BOX))
    finally:
        r.close()


@pytest.mark.gpu
def test_slot_source_equals_the_segment_and_does_not_follow_it(volumes):
    g = volumes["noise"]
    M = ragged(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        refused(lambda: r.histogram(source=3), "vx_histogram", "slot 3", "empty")
        r.set_segment_mask(M)
        r.store_segment(3)
        a = r.histogram(bins=128, source="segment", box=CUT_BOX)
        assert as_bytes(r.histogram(bins=128, source=3, box=CUT_BOX)) == as_bytes(a)
        same_histogram(a, region(d, M, CUT_BOX), 128, 0.0, 1.0)
        r.threshold(float(np.quantile(d, 0.9)))                               # the current segment moves on; the slot does not
        assert as_bytes(r.histogram(bins=128, source=3, box=CUT_BOX)) == as_bytes(a)
        assert as_bytes(r.histogram(bins=128, source="segment", box=CUT_BOX)) != as_bytes(a)
        r.drop_segment(3)
        refused(lambda: r.histogram(source=3), "empty")
    finally:
        r.close()


# ---- keys, order statistics, percentiles ------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_key_passes_and_order_statistics_are_np_sort(volumes):
    g = volumes["noise"]
    M = ragged(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        dr = d.ravel()
        # raw passes: no prefix, a prefix in the middle of the data (the top 11 bits of the key of the median of the positives),
        # one that nothing reaches, the last legal shapes
        mid = int(HR.order_key(np.array([np.median(dr[dr > 0])], F32))[0])
        for prefix, pb, b in ((0, 0, 11), (mid >> 21, 11, 11), (mid >> 10, 22, 10), (5, 11, 12), (mid >> 1, 31, 1), (mid >> 20, 12, 1)):
            counts, res = key_call(r, "volume", prefix, pb, b)
            want, below, above = HR.key_pass(dr, prefix, pb, b)
            assert np.array_equal(counts, want) and (res.below, res.above, res.count) == (below, above, dr.size), (prefix, pb, b)
            assert (res.d_sum, res.d_sum2, res.d_min, res.d_max) == (0.0, 0.0, 0.0, 0.0)        # moments = 0
        assert r.histogram_stats()[0] == 1 and r.histogram_stats()[2] == 0.0
        counts, res = key_call(r, "volume", mid >> 21, 11, 11, moments=1)
        assert below_above_nonzero(res) and res.d_sum > 0.0
        s = np.sort(dr)
        n = dr.size
        zeros = int((dr == 0).sum())
        assert zeros > 1000
        ranks = [0, n - 1, n // 2, zeros // 2, zeros - 1, zeros]
        got = r.density_order_statistic(ranks)
        assert got.dtype == np.float32 and np.array_equal(got.view(np.uint32), s[ranks].view(np.uint32))
        qs = [0, 25, 50, 75, 100]
        r.set_segment_mask(M)
        for kw, dd in ((dict(), dr), (dict(source="segment"), region(d, M)), (dict(box=CUT_BOX), region(d, box=CUT_BOX)),
                       (dict(source="segment", box=BOXES["inner"]), region(d, M, BOXES["inner"]))):
            got = r.density_percentile(qs, **kw)
            want = np.percentile(dd, qs, method="lower").astype(F32)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), kw
        med = r.density_percentile(50.0)
        assert isinstance(med, float) and F32(med) == np.percentile(dr, 50, method="lower")
        assert r.histogram_stats()[0] == 1                                  # the passes run without the moments' kernels
        with pytest.raises(ValueError, match="ranks"):
            r.density_order_statistic([n])
        r.set_segment_mask(np.zeros_like(M))
        refused(lambda: r.density_order_statistic([0], source="segment"), "density_order_statistic", "empty")
        refused(lambda: r.density_percentile(50, source="segment"), "density_percentile", "empty")
    finally:
        r.close()


def below_above_nonzero(res):
    return res.below > 0 and res.above > 0


# ---- layouts ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout_gives_the_same_bytes(volumes, layout):
    g = volumes["odd"]
    M = ragged(shape_of(g))
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("odd", g, p)
        same_histogram(r.histogram(bins=256), d.ravel(), 256, 0.0, 1.0, key=("odd", "all"))
        r.set_segment_mask(M)
        same_histogram(r.histogram(bins=50, range=(0.05, 0.6), source="segment", box=CUT_BOX), region(d, M, CUT_BOX), 50, 0.05, 0.6,
                       key=("odd", "ragged-cut"))
        got = r.density_percentile([10, 50, 99], source="segment")
        want = np.percentile(region(d, M), [10, 50, 99], method="lower").astype(F32)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    finally:
        r.close()


# ---- read-only ----------------------------------------------------------------------------------------------------------------------
VIEW = dict(mode="mip", size=(96, 64), dvr_step_voxels=0.5, dvr_jitter=False, max_samples=1 << 20, sample_range=(0.0, 1.0),
            dvr_skip_empty=True, use_env=False, show_environment=False)


@pytest.mark.gpu
def test_the_calls_change_nothing(volumes):
    g = volumes["noise"]
    M = ragged(shape_of(g))
    r = renderer(g, layout=LAYOUTS["brickf32"], **VIEW)
    try:
        r.set_segment_mask(M)
        r.store_segment(0)
        r.segment_edit("erode")
        r.store_segment(7)
        labels = r.islands(connectivity=26).labels()
        r.segment_distance(max_distance=6.0)
        field = r.distance_field()
        mask = SG.packed(r.segment_mask())
        slots = r.segments_labelmap([0, 7])
        off = frame(r)[0].copy()
        r.segment_view = "hide"
        hide = frame(r)[0].copy()
        r.render(frames=1, in_flight=1)
        accum, index = r.read_accum().copy(), r.frame_index
        c1 = r.counters()
        c1 = {f: getattr(c1, f) for f, _ in c1._fields_}
        stats = (r.segment_stats(), r.segment_edit_stats(), r.islands_stats(), r.distance_stats())
        for kw in (dict(), dict(source="segment"), dict(source=0, box=CUT_BOX)):
            r.histogram(bins=4096, **kw)
            r.density_percentile([5, 50, 95], **kw)
            r.otsu_threshold(**kw)
        c2 = r.counters()
        c2 = {f: getattr(c2, f) for f, _ in c2._fields_}
        assert c1 == c2 and r.frame_index == index and np.array_equal(r.read_accum().view(np.uint32), accum.view(np.uint32))
        assert stats == (r.segment_stats(), r.segment_edit_stats(), r.islands_stats(), r.distance_stats())
        assert r.segment_view == "hide" and r.stored_segments() == (0, 7)
        assert np.array_equal(SG.packed(r.segment_mask()), mask)
        assert np.array_equal(r.island_labels(), labels)                        # the table is still current ...
        assert np.array_equal(r.distance_field().view(np.uint32), field.view(np.uint32))    # ... and so is the field
        again = r.segments_labelmap([0, 7])
        assert np.array_equal(again[0], slots[0]) and again[1] == slots[1]
        assert np.array_equal(frame(r)[0].view(np.uint32), hide.view(np.uint32))
        r.segment_view = "off"
        assert np.array_equal(frame(r)[0].view(np.uint32), off.view(np.uint32))
    finally:
        r.close()


# ---- Otsu -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_otsu_threshold_on_the_phantom(volumes):
    g = volumes["phantom"]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("phantom", g, p)
        # (dyadic ranges: every edge is a float32 and the rule's products are exact, so d >= edge is the rule's own split)
        for bins, rng in ((256, (0.0, 1.0)), (32, (0.0, 0.5))):
            h = r.histogram(bins=bins, range=rng)
            k, want = HR.otsu(h.counts, *rng)                                   # the restatement on the device's own counts
            t = r.otsu_threshold(bins=bins, range=rng)
            assert k >= 0 and t == want == h.edges[k + 1]
            seg = r.threshold(t)                                                # the bright class: the bins above the split
            b = HR.linear_bins(d.ravel(), bins, *rng).reshape(d.shape)
            bright = d >= F32(t)
            assert seg.count == int(bright.sum()) and np.array_equal(r.segment_mask(), bright)
            assert int(h.counts[k + 1:].sum()) + h.above == seg.count
            assert np.array_equal(bright, ((b > k) & (b < bins)) | (b == bins + 1))
        refused(lambda: r.otsu_threshold(bins=4, range=(2.0, 3.0)), "otsu_threshold", "two non-empty bins")
    finally:
        r.close()


# ---- the C ABI --------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_c_refusals_name_the_field_and_change_nothing(volumes):
    from volxel_amd import _abi
    g = volumes["noise"]
    lib = _abi.load_library()
    n = 64 ** 3
    M = ragged((64, 64, 64))
    pm = SG.packed(M)
    back = np.zeros(n // 8, dtype=np.uint8)
    END = 0xffffffff

    def params(**kw):
        q = _abi.VxHistogramParams()
        q.source, q.slot, q.rule, q.bins, q.lo, q.hi, q.moments = 0, 0, 0, 256, 0.0, 1.0, 1
        q.box_lo[:], q.box_hi[:] = (0, 0, 0), (END, END, END)
        q.prefix, q.prefix_bits, q.key_bits = 0, 0, 11
        for k, v in kw.items():
            if k in ("box_lo", "box_hi"):
                getattr(q, k)[:] = v
            else:
                setattr(q, k, v)
        return q

    counts = np.full(4096, 77, dtype=np.uint64)
    res = _abi.VxHistogramResult()
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        err = lambda: lib.vx_last_error(ctx)
        call = lambda q, nc=256, cp=counts.ctypes.data: lib.vx_histogram(ctx, C.byref(q) if q is not None else None, cp, nc, C.byref(res))
        launches, ms = C.c_uint32(9), (C.c_double * 2)(1.0, 1.0)
        assert lib.vx_histogram_stats(ctx, C.byref(launches), ms) == 0 and (launches.value, ms[0], ms[1]) == (0, 0.0, 0.0)
        assert call(params()) == 3 and b"no volume" in err()                                             # VX_ERR_NO_VOLUME
        assert upload_volume(lib, ctx, g) == 0
        assert call(params()) == 1 and b"vx_set_params" in err()
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
            d = densities("noise", g, p)
        finally:
            r.close()
        assert lib.vx_resize(ctx, 64, 48) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        # VOLUME needs no segment: the first segment call of this context comes later
        assert call(params()) == 0 and np.array_equal(counts[:256], HR.linear(d.ravel(), 256, 0.0, 1.0)[0]) and res.count == n
        assert (counts[256:] == 77).all()                                                                # nothing written beyond the bins
        assert call(params(source=1)) == 1 and b"no current segment" in err()
        assert call(params(source=2, slot=4)) == 1 and b"empty" in err()
        assert lib.vx_segment_write_mask(ctx, pm.ctypes.data, n // 8, None) == 0
        assert lib.vx_segment_store(ctx, 4) == 0
        assert call(params(source=1)) == 0 and res.count == int(M.sum())
        want = res.count, res.d_sum
        assert call(params(source=2, slot=4)) == 0 and (res.count, res.d_sum) == want
        before = counts.copy()

        def refuse(rc, *words):
            assert rc == 1, (words, err())
            for w in words:
                assert w in err(), (w, err())
            assert b"vx_histogram" in err()
            occ = C.c_uint32()
            assert lib.vx_segment_read_mask(ctx, back.ctypes.data, n // 8) == 0 and np.array_equal(back, pm), words
            assert lib.vx_segment_slots(ctx, C.byref(occ)) == 0 and occ.value == 1 << 4, words
            assert np.array_equal(counts, before), words

        refuse(call(None), b"params")
        for bad in (-1, 3, 100):
            refuse(call(params(source=bad)), b"source")
        for bad in (-1, 2):
            refuse(call(params(rule=bad)), b"rule")
        for bad in (32, 33, END):
            refuse(call(params(source=2, slot=bad)), b"slot")
        refuse(call(params(source=2, slot=5)), b"slot 5", b"empty")
        refuse(call(params(box_lo=(5, 0, 0), box_hi=(4, END, END))), b"box")                             # an empty box
        refuse(call(params(box_hi=(63, 64, 63))), b"box")                                                # outside the volume
        refuse(call(params(box_lo=(0, 0, 64))), b"box")
        for bad in (0, 4097, END):
            refuse(call(params(bins=bad), nc=bad), b"bins")
        for lo, hi, word in ((math.nan, 1.0, b"lo"), (-math.inf, 1.0, b"lo"), (0.0, math.inf, b"hi"), (0.0, math.nan, b"hi"),
                             (0.5, 0.5, b"lo"), (0.75, 0.5, b"lo")):
            refuse(call(params(lo=lo, hi=hi)), word)
        refuse(call(params(lo=0.0, hi=1e-44, bins=4096), nc=4096), b"hi - lo")                           # inv would not be finite
        for bad in (0, 13, END):
            refuse(call(params(rule=1, key_bits=bad), nc=2048), b"key_bits")
        refuse(call(params(rule=1, prefix_bits=32, key_bits=1), nc=2), b"prefix_bits")
        refuse(call(params(rule=1, prefix_bits=22, key_bits=11), nc=2048), b"prefix_bits + key_bits")
        refuse(call(params(rule=1, prefix_bits=0, prefix=1), nc=2048), b"prefix")
        refuse(call(params(rule=1, prefix_bits=11, prefix=2048), nc=2048), b"prefix")
        for wrong in (255, 257, 0):
            refuse(call(params(), nc=wrong), b"ncounts")
        refuse(call(params(rule=1), nc=256), b"ncounts")                                                 # 2^11 bins, not 256
        refuse(call(params(), cp=None), b"counts")
        for bad in (-1, 2):
            refuse(call(params(moments=bad)), b"moments")
        # what is legal: a NULL result, the far-face marker, the largest shapes; then a valid call still succeeds
        assert lib.vx_histogram(ctx, C.byref(params()), counts.ctypes.data, 256, None) == 0
        assert call(params(rule=1, prefix_bits=31, prefix=0x7fffffff, key_bits=1), nc=2) == 0
        assert call(params(rule=1, prefix_bits=20, prefix=0xfffff, key_bits=12), nc=4096) == 0
        assert call(params(bins=4096), nc=4096) == 0 and np.array_equal(counts, HR.linear(d.ravel(), 4096, 0.0, 1.0)[0])
        assert lib.vx_histogram_stats(ctx, C.byref(launches), ms) == 0 and launches.value == 2 and ms[0] > 0.0
        assert lib.vx_histogram_stats(ctx, None, None) == 0
        assert upload_volume(lib, ctx, g) == 0                                                           # an upload drops the segment
        assert call(params(source=1)) == 1 and b"no current segment" in err()
        assert call(params(source=2, slot=4)) == 1 and b"empty" in err()
        assert call(params()) == 0 and res.count == n
    finally:
        lib.vx_destroy(ctx)


# ---- device groups and the JS host --------------------------------------------------------------------------------------------------
def chain(r, M):
    """what the group and the JS host must repeat"""
    r.set_segment_mask(M)
    r.store_segment(2)
    return (r.histogram(bins=128, range=(0.0, 0.5)), r.histogram(bins=16, source="segment", box=CUT_BOX),
            r.density_percentile([0, 25, 50, 75, 100], source=2), r.density_order_statistic([0, 1000]),
            r.otsu_threshold(bins=64), r.otsu_threshold(bins=32, source="segment"))


@pytest.mark.gpu
def test_device_group_answers_from_member0(volumes):
    g = volumes["odd"]
    M = ragged(shape_of(g))
    out = []
    for devices in (None, [0, 0]):
        r = renderer(g, devices=devices, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
            out.append(chain(r, M) + (r.histogram_stats()[0],))
        finally:
            r.close()
    d = densities("odd", g, p)
    same_histogram(out[0][0], d.ravel(), 128, 0.0, 0.5, key=("odd", "all"))
    for a, b in zip(*out):
        if hasattr(a, "counts"):
            assert as_bytes(a) == as_bytes(b)
        else:
            assert np.array_equal(np.asarray(a), np.asarray(b))


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_has_the_python_results(volumes, tmp_path):
    g = volumes["odd"]
    M = ragged(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        whole, seg, pct, order, otsu_all, otsu_seg = chain(r, M)
        med = r.density_percentile(50)
    finally:
        r.close()
    dump_grid(tmp_path, g)
    SG.packed(M).tofile(tmp_path / "m.bin")
    body = r"""
const before = r.histogramStats();
r.setSegmentMask(rd('m.bin', Uint8Array));
r.storeSegment(2);
const whole = r.histogram({ bins: 128, range: [0, 0.5] });
const seg = r.histogram({ bins: 16, source: 'segment', box: [[3, 0, 5], [60, 50, 63]] });
save('whole.bin', whole.counts); save('seg.bin', seg.counts); save('edges.bin', whole.edges);
const pct = r.densityPercentile([0, 25, 50, 75, 100], { source: 2 });
const order = r.densityOrderStatistic([0, 1000]);
save('pct.bin', pct); save('order.bin', order);
const med = r.densityPercentile(50);
const otsu = [r.otsuThreshold({ bins: 64 }), r.otsuThreshold({ bins: 32, source: 'segment' })];
const st = r.histogramStats();
const msg = (f) => { try { f(); return ''; } catch (e) { return String(e.message); } };
const refusals = [msg(() => r.histogram({ bins: 0 })), msg(() => r.histogram({ range: [1, 0] })), msg(() => r.histogram({ source: 'bone' })),
  msg(() => r.histogram({ source: 32 })), msg(() => r.histogram({ box: [[0, 0, 0], [64, 1, 1]] })), msg(() => r.densityPercentile(101)),
  msg(() => r.densityOrderStatistic([-1])), msg(() => r.densityOrderStatistic([1e9])), msg(() => r.histogram({ source: 9 })),
  msg(() => r.otsuThreshold({ bins: 4, range: [2, 3] }))];
const strip = (h) => { const o = Object.assign({}, h); delete o.counts; delete o.edges; return o; };
console.log(JSON.stringify({ before, whole: strip(whole), seg: strip(seg), med, otsu, st, refusals }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    for name, h in (("whole", whole), ("seg", seg)):
        js = out[name]
        got = np.fromfile(tmp_path / f"{name}.bin", dtype=np.float64)
        assert np.array_equal(got, h.counts.astype(np.float64))
        assert (js["count"], js["below"], js["above"]) == (h.count, h.below, h.above)
        assert (js["dSum"], js["dSum2"], js["mean"], js["std"]) == (h.d_sum, h.d_sum2, h.mean, h.std)
        assert F32(js["dMin"]) == F32(h.d_min) and F32(js["dMax"]) == F32(h.d_max)
    assert np.array_equal(np.fromfile(tmp_path / "edges.bin", dtype=np.float64), whole.edges)
    assert np.array_equal(np.fromfile(tmp_path / "pct.bin", dtype=np.uint32), pct.view(np.uint32))
    assert np.array_equal(np.fromfile(tmp_path / "order.bin", dtype=np.uint32), order.view(np.uint32))
    assert out["med"] == med and out["otsu"] == [otsu_all, otsu_seg]
    assert out["before"] == {"launches": 0, "histogramMs": 0, "momentsMs": 0} and out["st"]["launches"] == 2
    for text, word in zip(out["refusals"], ("bins", "range", "source", "source", "box", "q must be", "ranks", "ranks", "empty",
                                            "two non-empty bins")):
        assert word in text, (word, text)
