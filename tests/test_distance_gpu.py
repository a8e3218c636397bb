"""The distance field and the millimetre margins on the GPU (vx_segment_distance, vx_distance_read, vx_segment_margin; DESIGN.md
section 2 "Distances and margins") against the NumPy restatement (tests/distance_ref.py, itself pinned to the brute-force
definition and to SciPy by tests/test_distance_host.py): the field bit for bit on both sides, under three anisotropic spacings
and caps whose windows stay inside a brick, cross one brick boundary, cross two and do not exist, twice with identical bytes,
with its statistics exact; every margin op bit for bit with the mask's statistics; the unit margins against the voxel edits
run on the same device; a volume of three different extents; every layout; every tile width of the line passes; staleness, refusals, device groups, the masked
views, rendering left alone and the JS host."""
import ctypes as C
import json
import os
import shutil

import numpy as np
import pytest

from tests import distance_ref as DR
from tests import segment_ref as SG
from tests.common import F32, LAYOUTS, densities, frame, grid, renderer, segment_volumes, upload_volume
from tests.js_host import dump_grid, run_node
from tests.shapes import same_stats, shape_of, uploaded_shapes

SPACINGS = {"ct": (0.5, 0.5, 2.0), "ragged": (0.7, 0.9, 2.5), "mixed": (0.3, 1.1, 0.9)}
WINDOWS = (3, 9, 17, None)      # voxels on the coarsest axis: inside a brick, across one brick boundary, across two; no cap
SIDES = ("outside", "inside")


@pytest.fixture(scope="module")
def volumes():
    v = segment_volumes()
    return {"odd": v["odd"], "tube": v["tube"], "noise": v["noise"]}


def cap_for(window, sp):
    """a cap whose window on the coarsest axis is `window` voxels (wider on the finer axes)"""
    return np.inf if window is None else (window + 0.5) * max(sp)


def start_masks(shape):
    corner = np.zeros(shape, dtype=bool)
    corner[-1, 0, -1] = True
    return {"shapes": uploaded_shapes(shape), "corner": corner, "empty": np.zeros(shape, dtype=bool), "full": np.ones(shape, dtype=bool)}


_FIELDS = {}


def ref_field(vol, name, mask, side, sp):
    """the uncapped restatement of (volume, start mask, side, spacing), computed once per session and left unchanged"""
    key = (vol, name, side, sp)
    if key not in _FIELDS:
        f = DR.field(DR.source(mask, side), SPACINGS[sp])
        f.setflags(write=False)
        _FIELDS[key] = f
    return _FIELDS[key]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def check_field(r, vol, name, mask, side, sp, window):
    s, cap = SPACINGS[sp], cap_for(window, SPACINGS[sp])
    want = DR.capped(ref_field(vol, name, mask, side, sp), DR.cap2(cap))
    got = []
    for _ in range(2):
        res = r.segment_distance(side=side, max_distance=cap, spacing=s)
        got.append((r.distance_field(), res))
    (a, ra), (b, rb) = got
    assert a.dtype == np.float32 and a.shape == mask.shape
    assert np.array_equal(bits(a), bits(want)), (vol, name, side, sp, window, int((bits(a) != bits(want)).sum()))
    assert a.tobytes() == b.tobytes()
    fin, mx, arg = DR.stats(want, DR.source(mask, side), cap)
    for res in (ra, rb):
        assert (res.finite, F32(res.max_d2), res.argmax) == (fin, F32(mx), arg), (vol, name, side, sp, window, res.finite, res.max_d2, res.argmax)
        assert F32(res.max_distance) == np.sqrt(F32(mx))
    return want


CASES = [(v, m) for v in ("odd", "tube") for m in ("shapes", "corner", "empty", "full")]


@pytest.mark.gpu
@pytest.mark.parametrize("vol, name", CASES, ids=[f"{v}-{m}" for v, m in CASES])
def test_field_matches_the_restatement_bit_for_bit(volumes, vol, name):
    g = volumes[vol]
    mask = start_masks(shape_of(g))[name]
    r = renderer(g, dvr_jitter=False)
    try:
        r.set_segment_mask(mask)
        finite = 0
        for side in SIDES:
            for sp in sorted(SPACINGS):
                for window in WINDOWS:
                    want = check_field(r, vol, name, mask, side, sp, window)
                    finite += int(np.isfinite(want).sum())
                    if window is None and DR.source(mask, side).any():
                        assert np.isfinite(want).all()          # the uncapped field spans every line end to end
        assert finite > 0 or name in ("empty", "full")
        d = r.segment_distance(spacing=SPACINGS["ct"])
        assert np.array_equal(d.distance(), np.sqrt(d.squared())) and np.array_equal(r.segment_mask(), mask)   # M is not touched
        st = r.distance_stats()
        assert st[0] == 5 and all(t >= 0 for t in st[1:]) and len(st) == 5
    finally:
        r.close()


def slab_grid():
    """a 50 x 100 x 180 stack: the builder pads it to 64 x 128 x 192, three different brick counts (8, 16, 24), so x, y and z
    cannot stand in for one another anywhere; spacing (0.7, 0.9, 2.5)"""
    v = np.random.default_rng(12).integers(200, 3000, size=(180, 100, 50)).astype(np.uint16)
    return grid(v, SPACINGS["ragged"])


@pytest.mark.gpu
def test_three_different_extents(volumes):
    """every other volume here has Y = Z: on 64 x 128 x 192 a y-for-z swap in the passes' strides, the brick decode of the
    compare and the reduction, or the argmax shows"""
    g = slab_grid()
    shape = shape_of(g)
    assert shape == (192, 128, 64)
    masks = start_masks(shape)
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = SG.densities(g, p.volume_density_scale, p.volume_inv_maj)
        m0 = masks["shapes"]
        r.set_segment_mask(m0)
        check_field(r, "slab", "shapes", m0, "outside", "ragged", 9)
        check_field(r, "slab", "shapes", m0, "outside", "ragged", None)
        check_field(r, "slab", "shapes", m0, "inside", "mixed", 9)
        check_field(r, "slab", "shapes", m0, "inside", "mixed", None)
        assert len({tuple(r.segment_distance(side, spacing=SPACINGS["mixed"]).argmax) for side in SIDES}) == 2
        # one voxel in the corner (x = 63, y = 0, z = 191): the furthest voxel is the opposite corner, three different coordinates
        r.set_segment_mask(masks["corner"])
        check_field(r, "slab", "corner", masks["corner"], "outside", "ct", None)
        far = r.segment_distance(spacing=SPACINGS["ct"])
        assert far.argmax == (0, 127, 0) and far.finite == m0.size
        for op, radius in (("close", 5.0), ("grow", 9.5 * 2.5)):
            r.set_segment_mask(m0)
            seg = r.segment_margin(op, radius, spacing=SPACINGS["ragged"])
            want = DR.margin(m0, op, radius, SPACINGS["ragged"])
            assert np.array_equal(SG.packed(r.segment_mask()), SG.packed(want)) and (want ^ m0).any()
            same_stats(seg, want, d)
    finally:
        r.close()


def test_the_cases_reach_the_seams_they_name():
    """CPU: the caps give windows of 3, 9 and 17 voxels on the coarsest axis (no narrower on the others), and the corner voxel
    leaves rows of the padded tube (1088 x 64 x 64) empty and its own row with the nearest set voxel 135 bricks away"""
    for sp in SPACINGS.values():
        for w in (3, 9, 17):
            axis = int(np.argmax(sp))
            assert DR.window(sp[axis], DR.cap2(cap_for(w, sp)), 64) == w
            assert all(DR.window(sp[a], DR.cap2(cap_for(w, sp)), 4096) >= w for a in range(3))
    corner = start_masks((64, 64, 1088))["corner"]
    x = DR.x_pass_by_index(corner, 0.5)
    assert np.isinf(x[0, 0]).all() and x[-1, 0, 0] == DR.term(1087, 0.5)


RADII = (0.6, 9.5, 17.5)        # in voxels of the coarsest axis: under one voxel, past one brick, past two


# (the tube is 4.5 M voxels with its padding: one spacing and the longest reach, 17.5 voxels of 2.5 = 62 voxels of 0.7 along x)
@pytest.mark.gpu
@pytest.mark.parametrize("vol, sps, radii", [("odd", ("ct", "mixed", "ragged"), RADII), ("tube", ("ragged",), RADII[2:])],
                         ids=["odd", "tube"])
def test_every_margin_op_matches_the_restatement(volumes, vol, sps, radii):
    g = volumes[vol]
    m0 = uploaded_shapes(shape_of(g))
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities(vol, g, p)
        changed = 0
        for sp in sps:
            s = SPACINGS[sp]
            for k in radii:
                radius = k * max(s)
                for op in DR.OPS:
                    want = DR.margin(m0, op, radius, s)
                    sums = []
                    for _ in range(2):
                        r.set_segment_mask(m0)
                        seg = r.segment_margin(op, radius, spacing=s)
                        got = r.segment_mask()
                        assert np.array_equal(SG.packed(got), SG.packed(want)), (vol, sp, k, op, int(got.sum()), int(want.sum()))
                        same_stats(seg, want, d)
                        assert seg.rounds == 0 and seg.brick_visits == 0
                        sums.append(seg.d_sum)
                    assert sums[0] == sums[1]
                    changed += int((want ^ m0).sum())
                    st = r.distance_stats()
                    assert st[0] == (8 if op in ("open", "close") else 4) and all(t >= 0 for t in st[1:])
        assert changed > 0
        zero, one = np.zeros_like(m0), np.ones_like(m0)
        for op in DR.OPS:                                   # the empty set grows to itself, the whole volume shrinks to itself
            r.set_segment_mask(zero)
            assert r.segment_margin(op, 3.0, spacing=SPACINGS["ct"]).count == 0 and not r.segment_mask().any()
            r.set_segment_mask(one)
            assert r.segment_margin(op, 3.0, spacing=SPACINGS["ct"]).count == one.size and r.segment_mask().all()
    finally:
        r.close()


@pytest.mark.gpu
def test_grow_with_band_and_the_default_spacing(volumes):
    from volxel_amd import VolxelError
    g = volumes["odd"]                  # spacing (1.0, 1.2, 0.9) in its grid transform
    r = renderer(g, dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("odd", g, p)
        lo, hi = float(np.quantile(d[d > 0], 0.5)), float(np.quantile(d[d > 0], 0.97))
        pred = SG.predicate(d, lo, hi)
        core = uploaded_shapes(shape_of(g))
        from volxel_amd import _checks
        sp = _checks.spacing(None, r.volume.grid.transform)         # what spacing=None stands for
        assert np.allclose(sp, (1.0, 1.2, 0.9), rtol=1e-6)
        r.set_segment_mask(core)
        with pytest.raises(VolxelError, match="band"):       # no predicate on this volume yet
            r.segment_margin("grow", 2.0, band=True)
        assert np.array_equal(r.segment_mask(), core)
        r.threshold(lo, hi)
        assert np.array_equal(r.segment_mask(), pred)
        for radius in (0.95, 2.0, 10.3):
            r.set_segment_mask(core)
            seg = r.segment_margin("grow", radius, band=True)                       # spacing=None: the grid's own
            want = DR.margin(core, "grow", radius, sp, band=pred)
            got = r.segment_mask()
            assert np.array_equal(got, want) and not (got & ~core & ~pred).any() and (got & ~core).any()
            assert not np.array_equal(want, DR.margin(core, "grow", radius, sp))     # the band matters
            same_stats(seg, want, d)
            r.set_segment_mask(core)
            r.segment_margin("grow", radius)
            assert np.array_equal(r.segment_mask(), DR.margin(core, "grow", radius, sp))
        r.set_segment_mask(core)
        dist = r.segment_distance("inside")
        want = DR.field(~core, sp)
        assert np.array_equal(bits(dist.squared()), bits(want)) and dist.spacing == sp
        # the largest inscribed ball: its centre is in the segment and no nearer than its radius to any voxel outside it
        x, y, z = dist.argmax
        assert dist.max_d2 == float(want.max()) > 0 and r.segment_mask()[z, y, x]
    finally:
        r.close()


@pytest.mark.gpu
def test_unit_margins_are_the_voxel_edits_on_the_device(volumes):
    g = volumes["odd"]
    m0 = uploaded_shapes(shape_of(g))
    one = (1.0, 1.0, 1.0)
    r = renderer(g, dvr_jitter=False)
    try:
        def edited(op, conn):
            r.set_segment_mask(m0)
            r.segment_edit(op, steps=1, connectivity=conn)
            return r.segment_mask()

        def margined(op, radius, start=m0, sp=one):
            r.set_segment_mask(start)
            r.segment_margin(op, radius, spacing=sp)
            return r.segment_mask()

        assert np.array_equal(margined("grow", 1.0), edited("dilate", 6))
        assert np.array_equal(margined("grow", 1.75), edited("dilate", 26))
        assert np.array_equal(margined("shrink", 1.0), edited("erode", 6))
        assert np.array_equal(margined("shrink", 1.75), edited("erode", 26))
        assert (edited("dilate", 6) ^ edited("dilate", 26)).any()
        for sp in (one, SPACINGS["ct"]):
            radius = 2.2 * max(sp)
            c, o = margined("close", radius, sp=sp), margined("open", radius, sp=sp)
            assert not (m0 & ~c).any() and not (o & ~m0).any() and (c ^ m0).any() and (o ^ m0).any()
            assert np.array_equal(margined("close", radius, start=c, sp=sp), c)
            assert np.array_equal(margined("open", radius, start=o, sp=sp), o)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_layout_gives_the_same_field_and_margin(volumes, layout):
    """only the statistics of a margin's mask read the volume"""
    g = volumes["odd"]
    m0 = start_masks(shape_of(g))["shapes"]
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        p = r.bind_uniforms()
        d = densities("odd", g, p)
        r.set_segment_mask(m0)
        check_field(r, "odd", "shapes", m0, "outside", "ragged", 9)
        check_field(r, "odd", "shapes", m0, "inside", "ct", None)
        seg = r.segment_margin("close", 5.0, spacing=SPACINGS["ragged"])
        want = DR.margin(m0, "close", 5.0, SPACINGS["ragged"])
        assert np.array_equal(r.segment_mask(), want)
        same_stats(seg, want, d)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("lds_bytes", [4096, 2048, 1024, 512, 256])
def test_every_tile_width_of_the_line_passes(volumes, lds_bytes):
    """VX_DIST_LDS_BYTES (read when a context is created) shrinks the LDS budget of a tile: the volume's 64-voxel lines then
    take tiles of 16, 8, 4, 2 and 1 columns, the widths long lines get"""
    g = volumes["odd"]
    m0 = start_masks(shape_of(g))["shapes"]
    os.environ["VX_DIST_LDS_BYTES"] = str(lds_bytes)
    try:
        r = renderer(g, dvr_jitter=False)
    finally:
        del os.environ["VX_DIST_LDS_BYTES"]
    try:
        r.set_segment_mask(m0)
        check_field(r, "odd", "shapes", m0, "outside", "mixed", None)
        check_field(r, "odd", "shapes", m0, "inside", "ragged", 9)
        r.segment_margin("open", 4.0, spacing=SPACINGS["ct"])
        assert np.array_equal(r.segment_mask(), DR.margin(m0, "open", 4.0, SPACINGS["ct"]))
    finally:
        r.close()


@pytest.mark.gpu
def test_a_changed_mask_drops_the_field(volumes):
    from volxel_amd import VolxelError
    g = volumes["noise"]
    m0 = start_masks(shape_of(g))["shapes"]
    r = renderer(g, dvr_jitter=False)
    try:
        with pytest.raises(VolxelError, match="no current segment"):
            r.segment_distance()
        with pytest.raises(VolxelError, match="no current segment"):
            r.segment_margin("grow", 1.0)
        with pytest.raises(VolxelError, match="no current field"):
            r.distance_field()
        r.set_segment_mask(m0)
        with pytest.raises(VolxelError, match="no current field"):
            r.distance_field()

        def fresh():
            r.set_segment_mask(m0)
            d = r.segment_distance(max_distance=4.0, spacing=(1.0, 1.0, 1.0))
            assert np.array_equal(bits(d.squared()), bits(DR.field(m0, (1.0, 1.0, 1.0), 4.0)))
            return d

        changes = {
            "upload": lambda: (r.setup_from_grid(g), r.set_segment_mask(m0)),
            "segment": lambda: r.segment((10, 10, 10), 0.2, connectivity=26),
            "threshold": lambda: r.threshold(0.2),
            "segment_edit": lambda: r.segment_edit("dilate"),
            "segment_margin": lambda: r.segment_margin("grow", 1.0),
            "set_segment_mask": lambda: r.set_segment_mask(m0),
            "keep_largest_islands": lambda: r.keep_largest_islands(1),
        }
        for name, change in changes.items():
            d = fresh()
            change()
            with pytest.raises(VolxelError, match="no current field"):
                d.squared()
        d = fresh()                                  # what does not change the mask keeps the field
        r.islands()
        r.segment_mask()
        r.extract_mesh(segment=True)
        assert np.array_equal(bits(d.squared()), bits(DR.field(m0, (1.0, 1.0, 1.0), 4.0)))
        r.islands()
        r.segment_margin("close", 2.0)               # a margin drops the island table where an edit does
        with pytest.raises(VolxelError, match="no current table"):
            r.island_table(0, 1)
    finally:
        r.close()


@pytest.mark.gpu
def test_c_refusals_name_the_field_and_change_nothing(volumes):
    from volxel_amd import _abi
    g = volumes["noise"]
    lib = _abi.load_library()
    n = 64 ** 3
    m = uploaded_shapes((64, 64, 64))
    packed = SG.packed(m)
    back = np.zeros(n // 8, dtype=np.uint8)
    field = np.zeros(n, dtype=np.float32)
    seg, res = _abi.VxSegmentResult(), _abi.VxDistanceResult()
    dq, mq = _abi.VxDistanceParams(), _abi.VxMarginParams()
    dq.spacing[:], dq.max_distance, dq.side = (1.0, 1.0, 1.0), 3.0, 0
    mq.op, mq.radius, mq.band = 0, 2.0, 0
    mq.spacing[:] = (1.0, 1.0, 1.0)
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        err = lambda: lib.vx_last_error(ctx)
        assert lib.vx_segment_distance(ctx, C.byref(dq), C.byref(res)) == 3                             # VX_ERR_NO_VOLUME
        assert lib.vx_segment_margin(ctx, C.byref(mq), C.byref(seg)) == 3
        assert lib.vx_distance_read(ctx, field.ctypes.data, n) == 1 and b"no current field" in err()
        assert lib.vx_distance_stats(ctx, None, None) == 0
        assert upload_volume(lib, ctx, g) == 0
        assert lib.vx_segment_distance(ctx, C.byref(dq), C.byref(res)) == 1 and b"vx_set_params" in err()
        assert lib.vx_segment_margin(ctx, C.byref(mq), C.byref(seg)) == 1 and b"vx_set_params" in err()
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_resize(ctx, 64, 48) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        assert lib.vx_segment_distance(ctx, None, C.byref(res)) == 1 and b"params" in err()
        assert lib.vx_segment_margin(ctx, None, C.byref(seg)) == 1 and b"params" in err()
        assert lib.vx_segment_distance(ctx, C.byref(dq), C.byref(res)) == 1 and b"no current segment" in err()
        assert lib.vx_segment_margin(ctx, C.byref(mq), C.byref(seg)) == 1 and b"no current segment" in err()
        assert lib.vx_segment_write_mask(ctx, packed.ctypes.data, n // 8, C.byref(seg)) == 0
        assert lib.vx_segment_distance(ctx, C.byref(dq), None) == 0                                      # out may be NULL
        want = DR.field(m, (1.0, 1.0, 1.0), 3.0)

        def unchanged(what):
            assert lib.vx_segment_read_mask(ctx, back.ctypes.data, n // 8) == 0 and np.array_equal(back, packed), what
            assert lib.vx_distance_read(ctx, field.ctypes.data, n) == 0, what
            assert np.array_equal(bits(field), bits(want.ravel())), what

        def refused(fn, proto, word, **kw):
            q = type(proto).from_buffer_copy(proto)
            for k, v in kw.items():
                if k == "spacing":
                    q.spacing[:] = v
                else:
                    setattr(q, k, v)
            assert fn(ctx, C.byref(q), None) == 1, kw
            assert word in err(), (kw, err())
            unchanged(kw)

        nan, inf = float("nan"), float("inf")
        for fn, proto in ((lib.vx_segment_distance, dq), (lib.vx_segment_margin, mq)):
            for a in range(3):
                for bad in (0.0, -1.0, nan, inf):
                    sp = [1.0, 1.0, 1.0]
                    sp[a] = bad
                    refused(fn, proto, b"spacing[%d]" % a, spacing=tuple(sp))
        for bad in (0.0, -2.0, nan, -inf):
            refused(lib.vx_segment_distance, dq, b"max_distance", max_distance=bad)
        for bad in (-1, 2, 100):
            refused(lib.vx_segment_distance, dq, b"side", side=bad)
        for bad in (0.0, -2.0, nan, inf):
            refused(lib.vx_segment_margin, mq, b"radius", radius=bad)
        for bad in (-1, 4, 100):
            refused(lib.vx_segment_margin, mq, b"op", op=bad)
        for bad in (-1, 2):
            refused(lib.vx_segment_margin, mq, b"band", band=bad)
        for op in (1, 2, 3):
            refused(lib.vx_segment_margin, mq, b"band", op=op, band=1)
        refused(lib.vx_segment_margin, mq, b"band", band=1)                                              # no predicate on this volume
        assert lib.vx_distance_read(ctx, None, n) == 1 and b"d2" in err()
        for wrong in (n - 1, n + 1, 0):
            assert lib.vx_distance_read(ctx, field.ctypes.data, wrong) == 1 and b"nvoxels" in err()
        dq.max_distance = inf                                                                            # +inf is the uncapped field
        assert lib.vx_segment_distance(ctx, C.byref(dq), C.byref(res)) == 0 and res.finite == n
        assert lib.vx_segment_margin(ctx, C.byref(mq), None) == 0                                        # out may be NULL
        assert lib.vx_segment_read_mask(ctx, back.ctypes.data, n // 8) == 0
        assert np.array_equal(back, SG.packed(DR.margin(m, "grow", 2.0, (1.0, 1.0, 1.0))))
        assert lib.vx_distance_read(ctx, field.ctypes.data, n) == 1 and b"no current field" in err()
        launches, ms = C.c_uint32(), (C.c_double * 4)()
        assert lib.vx_distance_stats(ctx, C.byref(launches), ms) == 0 and launches.value == 4 and all(t >= 0 for t in ms)
        assert upload_volume(lib, ctx, g) == 0                                                           # an upload drops segment and field
        assert lib.vx_segment_distance(ctx, C.byref(dq), C.byref(res)) == 1 and b"no current segment" in err()
    finally:
        lib.vx_destroy(ctx)


@pytest.mark.gpu
def test_device_group_answers_from_member0(volumes):
    g = volumes["odd"]
    m0 = start_masks(shape_of(g))["shapes"]
    s = SPACINGS["ragged"]
    out = []
    for devices in (None, [0, 0]):
        r = renderer(g, devices=devices, dvr_jitter=False)
        try:
            r.set_segment_mask(m0)
            d = r.segment_distance("inside", max_distance=6.0, spacing=s)
            f = d.squared()
            seg = r.segment_margin("open", 4.0, spacing=s)
            out.append((f, (d.finite, d.max_d2, d.argmax), r.segment_mask(), (seg.count, seg.bbox_lo, seg.bbox_hi, seg.d_sum),
                        r.distance_stats()))
        finally:
            r.close()
    (fa, da, ma, sa, _), (fb, db, mb, sb, st) = out
    assert fa.tobytes() == fb.tobytes() and da == db and np.array_equal(ma, mb) and sa == sb
    assert np.array_equal(bits(fa), bits(DR.field(~m0, s, 6.0))) and np.array_equal(ma, DR.margin(m0, "open", 4.0, s))
    assert st[0] == 8 and all(t >= 0 for t in st[1:])


@pytest.mark.gpu
def test_segment_view_after_a_margin_matches_the_segview_restatement(volumes):
    """the MIP of the view "only" after a margin is, bit for bit, the projection of the volume whose voxels outside the
    restatement's mask decode to 0, with its counters (tests/segview_ref.py)"""
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
        r.segment_view = "only"
        before = frame(r)[0].copy()
        s = (0.8, 0.8, 1.5)
        r.segment_margin("close", 2.0, spacing=s)
        em = r.segment_mask()
        assert np.array_equal(em, DR.margin(m0, "close", 2.0, tuple(float(F32(v)) for v in s))) and (em ^ m0).any()
        assert r.frame_index == 0                       # the host restarted accumulation: the picture changed
        img = frame(r)[0]
        c = r.counters()
        tf, L = r._tf
        want, n, ntf, rays = SV.projection_image(r._params, g, tf, L, em, "only")
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
        st, est = r.segment_stats(), r.segment_edit_stats()
        r.segment_distance()
        r.segment_distance("inside", max_distance=3.0, spacing=SPACINGS["ct"]).squared()
        for op in DR.OPS:
            r.segment_margin(op, 1.5)
        b = r.read_accum().copy()
        c2 = r.counters()
        c2 = {f: getattr(c2, f) for f, _ in c2._fields_}
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert c1 == c2 and r.frame_index == 2
        assert r.segment_stats() == st and r.segment_edit_stats() == est
        r.render(frames=1, in_flight=1)           # accumulation goes on where it was
        assert r.counters().frames == c1["frames"] + 1 and r.frame_index == 3
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_has_the_python_bytes(volumes, tmp_path):
    g = volumes["odd"]
    m0 = start_masks(shape_of(g))["shapes"]
    s = SPACINGS["ragged"]
    r = renderer(g, dvr_jitter=False)
    try:
        r.set_segment_mask(m0)
        d = r.segment_distance("outside", max_distance=7.0, spacing=s)
        f = d.squared()
        d0 = r.segment_distance("inside")                       # the grid's own spacing
        seg = r.segment_margin("close", 4.0, spacing=s)
        m1 = r.segment_mask()
    finally:
        r.close()
    dump_grid(tmp_path, g)
    SG.packed(m0).tofile(tmp_path / "in.bin")
    (tmp_path / "args.json").write_text(json.dumps({"spacing": list(s)}))
    body = r"""
const a = JSON.parse(fs.readFileSync(path.join(dir, 'args.json')));
r.setSegmentMask(rd('in.bin', Uint8Array));
const d = r.segmentDistance({ side: 'outside', maxDistance: 7.0, spacing: a.spacing });
save('f.bin', d.squared());
const d0 = r.segmentDistance({ side: 'inside' });
const seg = r.segmentMargin('close', 4.0, { spacing: a.spacing });
save('m1.bin', r.segmentMask());
let stale = '', refused = '';
try { d.squared(); } catch (e) { stale = String(e.message); }
try { r.segmentMargin('shrink', 1.0, { band: true }); } catch (e) { refused = String(e.message); }
const pick = (o) => ({ finite: o.finite, maxD2: o.maxD2, maxDistance: o.maxDistance, argmax: o.argmax });
console.log(JSON.stringify({ d: pick(d), d0: pick(d0), seg, st: r.distanceStats(), stale, refused }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert np.fromfile(tmp_path / "f.bin", dtype=np.float32).tobytes() == f.tobytes()
    assert np.array_equal(np.fromfile(tmp_path / "m1.bin", dtype=np.uint8), SG.packed(m1))
    for js, py in ((out["d"], d), (out["d0"], d0)):
        assert js["finite"] == py.finite and F32(js["maxD2"]) == F32(py.max_d2) and tuple(js["argmax"]) == py.argmax
        assert F32(js["maxDistance"]) == F32(py.max_distance)
    js = out["seg"]
    assert js["count"] == seg.count and tuple(js["bboxLo"]) == seg.bbox_lo and tuple(js["bboxHi"]) == seg.bbox_hi
    assert js["dSum"] == seg.d_sum and js["converged"] is True and js["rounds"] == 0
    assert out["st"]["launches"] == 8 and "no current field" in out["stale"] and "band" in out["refused"]
