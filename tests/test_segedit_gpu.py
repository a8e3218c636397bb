"""Segment edits on the GPU (vx_segment_edit, vx_segment_write_mask; DESIGN.md section 2 "Segment edits") against the SciPy
restatement (tests/segedit_ref.py): the packed mask bit for bit, count, bbox, min and max exact, the float64 sum within 1e-9
relative of math.fsum (the bound vx_segment carries) and identical over two runs -- every op, both connectivities and step
counts past one brick and past two, from vx_segment results and from uploaded masks; band dilation; the write / read round trip;
fill holes on the CT phantom's soft tissue; the slice overlay, the segment views and pick on an edited mask; rendering left
alone; refusals, staleness after an upload, device groups and the JS host."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest

from tests import segedit_ref as ER
from tests import segment_ref as SG
from tests.common import F32, LAYOUTS, densities, frame, renderer, segment_volumes, upload_volume
from tests.js_host import dump_grid, run_node
from tests.shapes import CASES, resolve, same_stats, shape_of, uploaded_shapes

STEPS = (1, 2, 3, 8, 9, 17)   # past one brick (8) and past two (17)
STEP_OPS = ("dilate", "erode", "open", "close")


@pytest.fixture(scope="module")
def volumes():
    return segment_volumes()


def _edit_twice(r, start, d, op, conn, n=1, band=None):
    """installs `start`, edits, reads back -- twice; the mask and the statistics against the restatement, the sum identical"""
    want = ER.edit(start, op, conn, n, band=band)
    got = []
    for _ in range(2):
        r.set_segment_mask(start)
        s = r.segment_edit(op, steps=1 if op == "fill_holes" else n, connectivity=conn, band=band is not None)
        m = r.segment_mask()
        assert np.array_equal(SG.packed(m), SG.packed(want)), (op, conn, n, int(m.sum()), int(want.sum()))
        same_stats(s, want, d)
        if op != "fill_holes":
            assert s.rounds == 0 and s.brick_visits == 0
        got.append(s)
    a, b = got
    assert (a.count, a.bbox_lo, a.bbox_hi, a.d_min, a.d_max, a.d_sum) == (b.count, b.bbox_lo, b.bbox_hi, b.d_min, b.d_max, b.d_sum)
    return got[0], want


# (volume, its vx_segment case of tests/shapes.py -- or None: a mask built on the host).  The stack with odd sides is
# mostly padding, so its case there (lo = the 0.55 quantile = 0) is the whole volume, which no edit changes: q0.9 here.
STARTS = {"noise": ("noise", CASES["noise_q70"]), "phantom": ("phantom", CASES["phantom_bone"]),
          "odd": ("odd", ("odd", "max", "q0.9", None, None)), "tube": ("tube", CASES["tube"]),
          "uploaded": ("odd", None), "uploaded_noise": ("noise", None)}


def _start(r, g, name):
    """the start mask of STARTS[name] (from vx_segment, or built on the host) and the densities"""
    vol, case = STARTS[name]
    p = r.bind_uniforms()
    d = densities(vol, g, p)
    if case is None:
        return uploaded_shapes(shape_of(g)), d
    _, seed, lo, hi, box = case
    seed, lo_v, hi_v, _ = resolve(d, seed, lo, hi, box)
    s = r.segment(seed, lo_v, hi_v, connectivity=6, box=box)
    assert s.count > 0
    return r.segment_mask(), d


@pytest.mark.gpu
@pytest.mark.parametrize("start", sorted(STARTS))
@pytest.mark.parametrize("conn", [6, 26])
def test_every_op_matches_the_restatement(volumes, start, conn):
    g = volumes[STARTS[start][0]]
    r = renderer(g, dvr_jitter=False)
    try:
        m0, d = _start(r, g, start)
        if STARTS[start][1] is not None:   # straight from vx_segment, without an upload in between
            s = r.segment_edit("dilate", steps=2, connectivity=conn)
            assert np.array_equal(r.segment_mask(), ER.edit(m0, "dilate", conn, 2))
            same_stats(s, ER.edit(m0, "dilate", conn, 2), d)
        changed = 0
        for op in STEP_OPS:
            for n in STEPS:
                _, want = _edit_twice(r, m0, d, op, conn, n)
                changed += int((want ^ m0).sum())
        _, want = _edit_twice(r, m0, d, "fill_holes", conn)
        assert not (m0 & ~want).any()
        assert changed > 0
        assert r.segment_edit_stats()[0] >= 3 and all(t >= 0 for t in r.segment_edit_stats()[1:])
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout_gives_the_same_edit(volumes, layout):
    """only the statistics read the volume"""
    g = volumes["odd"]
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        m0, d = _start(r, g, "odd")
        for op, conn, n in (("close", 26, 3), ("erode", 6, 2), ("dilate", 26, 9), ("fill_holes", 6, 1)):
            _edit_twice(r, m0, d, op, conn, n)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [6, 26])
def test_band_dilation(volumes, conn):
    from volxel_amd import VolxelError
    g = volumes["noise"]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        seed, lo, hi, pred = resolve(d, "max", "q0.6", "q0.95", ((3, 0, 5), (60, 50, 63)))
        box = ((3, 0, 5), (60, 50, 63))
        r.segment(seed, lo, hi, connectivity=6, box=box)
        m = r.segment_mask()
        # after a real vx_segment: shrink, then grow back inside the band only
        r.segment_edit("erode", steps=2, connectivity=6)
        core = r.segment_mask()
        assert 0 < core.sum() < m.sum()
        for n in (1, 3, 9):
            r.set_segment_mask(core)
            s = r.segment_edit("dilate", steps=n, connectivity=conn, band=True)
            want = ER.edit(core, "dilate", conn, n, band=pred)
            got = r.segment_mask()
            assert np.array_equal(got, want) and not (got & ~pred).any() and got.sum() > core.sum()
            if n >= 3:   # (one 6-step from a core eroded by 2 stays inside the old segment, hence inside P)
                assert not np.array_equal(want, ER.edit(core, "dilate", conn, n))   # the band matters here
            same_stats(s, want, d)
        # after a fill: the predicate words of vx_segment survive the fill's own flood
        r.set_segment_mask(core)
        r.segment_edit("fill_holes", connectivity=conn)
        filled = r.segment_mask()
        assert np.array_equal(filled, ER.edit(core, "fill_holes", conn))
        r.segment_edit("dilate", steps=2, connectivity=conn, band=True)
        assert np.array_equal(r.segment_mask(), ER.edit(filled, "dilate", conn, 2, band=pred))
        # an uploaded mask with voxels outside P: they stay
        out = core.copy()
        zz, yy, xx = np.nonzero(~pred)
        out[zz[:50], yy[:50], xx[:50]] = True
        out[0:2, 52:60, 0:2] = True          # outside the box
        assert (out & ~pred).sum() >= 50
        r.set_segment_mask(out)
        r.segment_edit("dilate", steps=3, connectivity=conn, band=True)
        got = r.segment_mask()
        assert np.array_equal(got, ER.edit(out, "dilate", conn, 3, band=pred))
        assert np.array_equal(got & ~pred, out & ~pred)
        # a new upload drops the predicate: a mask alone does not bring one back
        r.setup_from_grid(volumes["noise"])
        r.set_segment_mask(core)
        with pytest.raises(VolxelError, match="band"):
            r.segment_edit("dilate", connectivity=conn, band=True)
        assert np.array_equal(r.segment_mask(), core)
        r.segment_edit("dilate", connectivity=conn)
        assert np.array_equal(r.segment_mask(), ER.edit(core, "dilate", conn, 1))
    finally:
        r.close()


@pytest.mark.gpu
def test_write_read_round_trip_and_the_trivial_masks(volumes):
    g = volumes["odd"]                         # a 37 x 29 x 45 stack: the padding behind it is part of the mask
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("odd", g, p)
        shape = shape_of(g)
        assert shape[0] > 45 and shape[1] > 29 and shape[2] > 37
        m = np.random.default_rng(3).random(shape) < 0.37
        s = r.set_segment_mask(m)              # on a context that never ran vx_segment
        bits = np.empty(m.size // 8, dtype=np.uint8)
        assert r._lib.vx_segment_read_mask(r._ctx, bits.ctypes.data, bits.size) == 0
        assert np.array_equal(bits, SG.packed(m))
        assert m[45:].any() and m[:, 29:].any() and m[:, :, 37:].any()
        same_stats(s, m, d)
        assert s.rounds == 0 and s.brick_visits == 0
        assert r.set_segment_mask(m).d_sum == s.d_sum
        zero, one = np.zeros(shape, dtype=bool), np.ones(shape, dtype=bool)
        for conn in (6, 26):
            for op in ER.OPS:
                for n in ((1,) if op == "fill_holes" else (1, 9)):
                    r.set_segment_mask(zero)
                    s0 = r.segment_edit(op, steps=n, connectivity=conn)
                    assert not r.segment_mask().any()
                    assert (s0.count, s0.bbox_lo, s0.bbox_hi, s0.d_min, s0.d_max, s0.d_sum) == (0, (0, 0, 0), (0, 0, 0), 0.0, 0.0, 0.0)
                    s1 = r.set_segment_mask(one)
                    s2 = r.segment_edit(op, steps=n, connectivity=conn)
                    assert r.segment_mask().all() and s2.count == one.size == s1.count and s2.d_sum == s1.d_sum
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("conn", [6, 26])
def test_fill_holes_on_the_phantoms_soft_tissue_and_the_serpentine(volumes, conn):
    from volxel_amd import synth
    vox, _ = synth.ct_phantom(64)
    g = volumes["phantom"]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("phantom", g, p)
        lo, hi = float(d[vox >= 1000].min()), float(d[vox <= 1300].max())     # raw 1000 .. 1300: d is monotone in the raw value
        a = r.segment((32, 32, 32), lo, hi, connectivity=conn)
        m = r.segment_mask()
        assert a.count == 38090
        b = r.segment_edit("fill_holes", connectivity=conn)
        f = r.segment_mask()
        want = ER.edit(m, "fill_holes", conn)
        assert np.array_equal(f, want)
        assert b.count - a.count == 8538 and (b.bbox_lo, b.bbox_hi) == (a.bbox_lo, a.bbox_hi)   # lungs, spine and ribs
        assert b.rounds > 0 and b.brick_visits > 0 and b.converged
        same_stats(b, want, d)
        assert f[32, 32, 47] and not m[32, 32, 47]                              # inside a lung
        c = r.segment_edit("fill_holes", connectivity=conn)                     # idempotent
        assert c.count == b.count and np.array_equal(r.segment_mask(), f)
    finally:
        r.close()
    g = volumes["serpentine"]
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("serpentine", g, p)
        a = r.segment((0, 0, 0), float(d.max()) / 2, connectivity=conn)
        m = r.segment_mask()
        b = r.segment_edit("fill_holes", connectivity=conn)
        assert b.count == a.count > 1000 and np.array_equal(r.segment_mask(), m)   # nothing to fill
        assert np.array_equal(m, ER.edit(m, "fill_holes", conn))
    finally:
        r.close()


@pytest.mark.gpu
def test_overlay_views_and_pick_read_the_edited_mask(volumes):
    from volxel_amd import mpr
    g = volumes["phantom"]

    def bone(r):
        p = r.bind_uniforms()
        d = densities("phantom", g, p)
        seed, lo, hi, _ = resolve(d, "max", 0.75, None, None)
        r.segment(seed, lo, connectivity=6)
        return d

    r = renderer(g, layout=LAYOUTS["brickf32"], dvr_jitter=False)
    images = {}
    try:
        bone(r)
        m0 = r.segment_mask()
        r.segment_view = "only"
        r.segment_edit("dilate", steps=2, connectivity=26)
        em = r.segment_mask()
        assert np.array_equal(em, ER.edit(m0, "dilate", 26, 2))
        for sp in (mpr.axial(r, 30), mpr.coronal(r, 40),
                   mpr.oblique(r, (0.0, 0.05, 0.0), (0.0, 0.0, 1.0), (0, 1, 0), 0.008, (80, 80), thickness=0.2, samples=9)):
            assert np.array_equal(r.slice_mask(sp), SG.overlay(sp, em))
        for mode in ("dvr", "mip"):
            r.settings.render_mode = mode
            r.restart_rendering()
            r.render(frames=1, in_flight=1)
            images[mode] = r.read_accum().copy()
        # pick lands on the dilated surface: the hit's nearest voxel is in the edited mask, and some are outside the old one
        r.settings.render_mode = "dvr"
        _, hit = r.isosurface(0.5, refine=8)
        ys, xs = np.nonzero(hit[..., 3] >= 0)
        assert len(xs) > 50
        vis = [r.voxel_index(hit[y, x, :3]) for y, x in zip(ys[::7], xs[::7])]
        vis = [v for v in vis if v is not None]
        near = ER.edit(em, "dilate", 26, 1)    # the interpolated surface lies within a voxel of the mask
        assert vis and all(near[v[2], v[1], v[0]] for v in vis)
        assert any(not m0[v[2], v[1], v[0]] for v in vis)
    finally:
        r.close()
    r = renderer(g, layout=LAYOUTS["brickf32"], dvr_jitter=False)
    try:
        r.set_segment_mask(em)                 # a fresh renderer: the same mask installed from the host
        r.segment_view = "only"
        for mode in ("dvr", "mip"):
            r.settings.render_mode = mode
            r.restart_rendering()
            r.render(frames=1, in_flight=1)
            img = r.read_accum().copy()
            assert np.array_equal(img.view(np.uint32), images[mode].view(np.uint32)), mode
            assert img[..., :3].any()
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("view", ["only", "hide"])
def test_segment_view_of_an_edited_mask_matches_the_segview_restatement(volumes, view):
    """one small case against tests/segview_ref.py: the MIP of the view of an edited mask is, bit for bit, the projection of
    the volume whose hidden voxels decode to 0, with its counters"""
    from tests import segview_ref as SV
    g = volumes["noise"]
    r = renderer(g, layout=LAYOUTS["brickf32"], mode="mip", size=(96, 64), dvr_step_voxels=0.5, dvr_jitter=False,
                 max_samples=1 << 20, sample_range=(0.0, 1.0), dvr_skip_empty=True, use_env=False, show_environment=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        lo, hi = float(np.quantile(d, 0.6)), float(np.quantile(d, 0.95))
        z, y, x = np.unravel_index(int(np.argmax(np.where(SG.predicate(d, lo, hi), d, -np.inf))), d.shape)
        r.segment((int(x), int(y), int(z)), lo, hi, connectivity=6)
        m0 = r.segment_mask()
        r.segment_view = view
        before = frame(r)[0].copy()
        r.segment_edit("close", steps=2, connectivity=26)
        em = r.segment_mask()
        assert np.array_equal(em, ER.edit(m0, "close", 26, 2)) and (em ^ m0).any()
        assert r.frame_index == 0                       # the host restarted accumulation: the picture changed
        img = frame(r)[0]
        c = r.counters()
        tf, L = r._tf
        want, n, ntf, rays = SV.projection_image(r._params, g, tf, L, em, view)
        assert np.array_equal(img, want), float(np.abs(img - want).max())
        assert c.samples == n and c.skip_steps == 0 and c.tf_samples == ntf and c.rays == rays
        assert not np.array_equal(img, before)
    finally:
        r.close()


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
        frame = r.frame_index
        st = r.segment_stats()
        m = r.segment_mask()
        for op in ER.OPS:
            r.segment_edit(op, connectivity=26)
        r.set_segment_mask(m)
        b = r.read_accum().copy()
        c2 = r.counters()
        c2 = {f: getattr(c2, f) for f, _ in c2._fields_}
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert c1 == c2
        assert frame == r.frame_index == 2
        assert r.segment_stats() == st            # vx_segment_stats keeps reporting the last vx_segment
        r.render(frames=1, in_flight=1)           # accumulation goes on where it was
        assert r.counters().frames == c1["frames"] + 1 and r.frame_index == 3
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_leave_the_segment_alone(volumes):
    from volxel_amd import _abi
    g = volumes["noise"]
    lib = _abi.load_library()
    nbytes = 64 ** 3 // 8
    res = _abi.VxSegmentResult()
    q = _abi.VxSegmentEditParams()
    q.op, q.connectivity, q.steps, q.band = 0, 6, 1, 0
    m = ER.blobs((64, 64, 64), seed=5)
    bits = SG.packed(m)
    back = np.zeros(nbytes, dtype=np.uint8)
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.vx_segment_edit(ctx, C.byref(q), C.byref(res)) == 3                                   # VX_ERR_NO_VOLUME
        assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, nbytes, C.byref(res)) == 3
        assert lib.vx_segment_edit_stats(ctx, None, None) == 0
        assert upload_volume(lib, ctx, g) == 0
        assert lib.vx_segment_edit(ctx, C.byref(q), C.byref(res)) == 1 and b"vx_set_params" in lib.vx_last_error(ctx)
        assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, nbytes, None) == 1 and b"vx_set_params" in lib.vx_last_error(ctx)
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_resize(ctx, 64, 48) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        assert lib.vx_segment_edit(ctx, C.byref(q), C.byref(res)) == 1 and b"no current segment" in lib.vx_last_error(ctx)
        assert lib.vx_segment_write_mask(ctx, None, nbytes, C.byref(res)) == 1 and b"bits" in lib.vx_last_error(ctx)
        for wrong in (nbytes - 1, nbytes + 8, 0):
            assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, wrong, C.byref(res)) == 1 and b"nbytes" in lib.vx_last_error(ctx)
        assert lib.vx_segment_read_mask(ctx, back.ctypes.data, nbytes) == 1                              # still no segment
        assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, nbytes, C.byref(res)) == 0
        assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, nbytes, None) == 0
        count = res.count
        assert count == int(m.sum())

        def refused(word, **kw):
            b = _abi.VxSegmentEditParams.from_buffer_copy(q)
            for k, v in kw.items():
                setattr(b, k, v)
            out = _abi.VxSegmentResult()
            assert lib.vx_segment_edit(ctx, C.byref(b), C.byref(out)) == 1, kw
            assert word in lib.vx_last_error(ctx), (kw, lib.vx_last_error(ctx))
            assert lib.vx_segment_read_mask(ctx, back.ctypes.data, nbytes) == 0 and np.array_equal(back, bits), kw

        assert lib.vx_segment_edit(ctx, None, C.byref(res)) == 1 and b"params" in lib.vx_last_error(ctx)
        for op in (-1, 5, 100):
            refused(b"op", op=op)
        for cn in (0, 4, 8, 18, 27, -6):
            refused(b"connectivity", connectivity=cn)
        for n in (0, 1025, 0xFFFFFFFF):
            refused(b"steps", steps=n)
        refused(b"steps", op=4, steps=2)
        for bd in (-1, 2):
            refused(b"band", band=bd)
        for op in (1, 2, 3, 4):
            refused(b"band", op=op, band=1)
        refused(b"band", band=1)                                                                          # no predicate on this volume
        # the statistics are those of the mask still: an edit that changes nothing reports them
        b = _abi.VxSegmentEditParams.from_buffer_copy(q)
        b.op, b.steps = 4, 0
        filled = ER.edit(m, "fill_holes", 6)
        assert lib.vx_segment_edit(ctx, C.byref(b), C.byref(res)) == 0 and res.count == int(filled.sum()) and res.converged == 1
        assert lib.vx_segment_edit(ctx, C.byref(q), None) == 0                                            # out may be NULL
        assert lib.vx_segment_read_mask(ctx, back.ctypes.data, nbytes) == 0
        assert np.array_equal(back, SG.packed(ER.edit(filled, "dilate", 6, 1)))
        # an upload drops segment, predicate and scratch
        assert upload_volume(lib, ctx, g) == 0
        assert lib.vx_segment_edit(ctx, C.byref(q), C.byref(res)) == 1 and b"no current segment" in lib.vx_last_error(ctx)
        assert lib.vx_segment_write_mask(ctx, bits.ctypes.data, nbytes, C.byref(res)) == 0 and res.count == count
        assert lib.vx_segment_edit(ctx, C.byref(q), C.byref(res)) == 0
    finally:
        lib.vx_destroy(ctx)


@pytest.mark.gpu
def test_python_refusals_on_a_live_renderer(volumes):
    from volxel_amd import VolxelError
    r = renderer(volumes["noise"], dvr_jitter=False)
    try:
        with pytest.raises(VolxelError, match="no current segment"):
            r.segment_edit("dilate")
        with pytest.raises(ValueError, match="shape"):
            r.set_segment_mask(np.zeros((64, 64, 32), dtype=bool))
        with pytest.raises(ValueError, match="bool"):
            r.set_segment_mask(np.zeros((64, 64, 64), dtype=np.uint8))
    finally:
        r.close()


@pytest.mark.gpu
def test_device_group_runs_the_edits_on_member0(volumes):
    g = volumes["noise"]
    m = ER.blobs((64, 64, 64), seed=8)
    r1 = renderer(g, dvr_jitter=False)
    try:
        a0 = r1.set_segment_mask(m)
        a1 = r1.segment_edit("close", steps=3, connectivity=26)
        ma = r1.segment_mask()
        a2 = r1.segment_edit("fill_holes", connectivity=6)
        fa = r1.segment_mask()
    finally:
        r1.close()
    r2 = renderer(g, devices=[0, 0], dvr_jitter=False)
    try:
        b0 = r2.set_segment_mask(m)
        b1 = r2.segment_edit("close", steps=3, connectivity=26)
        mb = r2.segment_mask()
        b2 = r2.segment_edit("fill_holes", connectivity=6)
        fb = r2.segment_mask()
        st = r2.segment_edit_stats()
    finally:
        r2.close()
    assert np.array_equal(ma, mb) and np.array_equal(fa, fb) and np.array_equal(ma, ER.edit(m, "close", 26, 3))
    for a, b in ((a0, b0), (a1, b1), (a2, b2)):
        assert (a.count, a.bbox_lo, a.bbox_hi, a.d_min, a.d_max, a.d_sum) == (b.count, b.bbox_lo, b.bbox_hi, b.d_min, b.d_max, b.d_sum)
    assert st[0] >= 3 and all(t >= 0 for t in st[1:])


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_edits_have_the_python_bits(volumes, tmp_path):
    g = volumes["noise"]
    m = ER.blobs((64, 64, 64), seed=4)
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("noise", g, p)
        seed, lo, _, _ = resolve(d, "max", "q0.6", None, None)
        r.segment(seed, lo, connectivity=6)
        s1 = r.segment_edit("dilate", steps=3, connectivity=26)
        m1 = r.segment_mask()
        s2 = r.segment_edit("fill_holes", connectivity=6)
        m2 = r.segment_mask()
        s3 = r.set_segment_mask(m)
    finally:
        r.close()
    dump_grid(tmp_path, g)
    SG.packed(m).tofile(tmp_path / "in.bin")
    (tmp_path / "args.json").write_text(json.dumps({"seed": list(seed), "lo": lo}))
    body = r"""
const a = JSON.parse(fs.readFileSync(path.join(dir, 'args.json')));
r.segment(a.seed, a.lo, { connectivity: 6 });
const s1 = r.segmentEdit('dilate', { steps: 3, connectivity: 26 });
save('m1.bin', r.segmentMask());
const s2 = r.segmentEdit('fill_holes', { connectivity: 6 });
save('m2.bin', r.segmentMask());
const s3 = r.setSegmentMask(rd('in.bin', Uint8Array));
save('m3.bin', r.segmentMask());
let refused = '';
try { r.segmentEdit('erode', { band: true }); } catch (e) { refused = String(e.message); }
console.log(JSON.stringify({ s1, s2, s3, st: r.segmentEditStats(), refused }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert np.array_equal(np.fromfile(tmp_path / "m1.bin", dtype=np.uint8), SG.packed(m1))
    assert np.array_equal(np.fromfile(tmp_path / "m2.bin", dtype=np.uint8), SG.packed(m2))
    assert np.array_equal(np.fromfile(tmp_path / "m3.bin", dtype=np.uint8), SG.packed(m))
    for js, s in ((out["s1"], s1), (out["s2"], s2), (out["s3"], s3)):
        assert js["count"] == s.count and tuple(js["bboxLo"]) == s.bbox_lo and tuple(js["bboxHi"]) == s.bbox_hi
        assert F32(js["dMin"]) == F32(s.d_min) and F32(js["dMax"]) == F32(s.d_max) and js["dSum"] == s.d_sum
        assert js["converged"] is True
    assert out["s2"]["rounds"] > 0 and out["s1"]["rounds"] == 0
    assert "band" in out["refused"] and out["st"]["launches"] == 1
