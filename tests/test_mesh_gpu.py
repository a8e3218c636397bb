"""The GPU mesher (vx_mesh_extract, DESIGN.md section 2 "Meshes") against the NumPy restatement (tests/mesh_ref.py): after the
canonical sort the vertex floats (as uint32), the cells and the triangles are equal bit for bit -- every layout, the density
source at several iso (one a value some voxel equals exactly, one above the maximum) and the segment source (from vx_segment,
after a close, after an uploaded mask that touches all six faces), with the whole volume, an interior box, a one-voxel box and a
box on a brick boundary.  Two calls and every layout return the same raw bytes; VxMeshResult equals the restatement's counts;
rendering, the counters, the segment, its view and pick are left alone; refusals, staleness after an upload, a device group,
the JS host and the world-space conventions."""
import ctypes as C

import numpy as np
import pytest

from tests import mesh_ref as MR
from tests import segment_ref as SG
from tests.common import F32, LAYOUTS, densities, grid, renderer, segment_volumes, upload_volume
from tests.js_host import dump_grid, run_node

BOXES = {"whole": None, "interior": ((5, 9, 3), (40, 30, 37)), "one_voxel": ((17, 18, 19), (17, 18, 19)),
         "brick_boundary": ((8, 16, 0), (23, 31, 15))}


@pytest.fixture(scope="module")
def volumes():
    return segment_volumes()


def _raw(r, **kw):
    m = r.extract_mesh(space="voxel", **kw)
    return m.vertices.astype(F32), m.cells, m.triangles


def _same(got, want, what):
    gv, gc, gt = MR.canonical(*got)
    wv, wc, wt = MR.canonical(*want)
    assert gv.shape == wv.shape and gt.shape == wt.shape, (what, gv.shape, wv.shape, gt.shape, wt.shape)
    assert np.array_equal(gc, wc), what
    assert np.array_equal(np.ascontiguousarray(gv, dtype=F32).view(np.uint32), np.ascontiguousarray(wv, dtype=F32).view(np.uint32)), what
    assert np.array_equal(gt, wt), what


def _same_result(res, inside, box):
    want = MR.counts(inside, box)
    got = {"vertices": int(res.vertices), "triangles": int(res.triangles), "active_blocks": int(res.active_blocks),
           "blocks": int(res.blocks), "bbox_lo": tuple(int(np.int32(np.uint32(a))) for a in res.bbox_lo[:]),
           "bbox_hi": tuple(int(np.int32(np.uint32(a))) for a in res.bbox_hi[:])}
    assert got == want


def _isos(d):
    """a quantile, a value some voxel equals exactly (>= is exercised), a high one, and one above the maximum (empty)"""
    pos = d[d > 0]
    exact = float(pos.flat[len(pos.flat) // 3])
    return [float(np.quantile(pos, 0.5)), exact, float(np.quantile(pos, 0.97)), float(d.max()) * 1.5]


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("vol", ["noise", "phantom", "odd"])
def test_density_meshes_match_the_restatement_bit_for_bit(volumes, vol, layout):
    g = volumes[vol]
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        d = densities(vol, g, r.bind_uniforms())
        Z, Y, X = d.shape
        isos = _isos(d)
        assert (d == F32(isos[1])).any()
        for k, iso in enumerate(isos):
            for name, box in BOXES.items():
                if box is not None and not all(h < e for h, e in zip(box[1], (X, Y, Z))):
                    continue
                got = _raw(r, iso=iso, box=box)
                _same(got, MR.extract_density(d, iso, box), (vol, layout, iso, name))
                _same_result(r.last_mesh_result, d >= F32(iso), box)
                if k == 3:
                    assert len(got[0]) == 0 and len(got[2]) == 0
                again = _raw(r, iso=iso, box=box)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
    finally:
        r.close()


def _touching_all_faces(shape):
    Z, Y, X = shape
    rng = np.random.default_rng(21)
    m = rng.random(shape) < 0.08
    m[:3, :3, :3] = True
    m[Z - 4:, Y - 4:, X - 4:] = True
    m[6:11, 6:11, 6:11] = True
    m[16, 9:23, 3:X - 2] = True
    m[:, Y // 2, X // 2] = True
    m[Z // 2, :, X // 3] = True
    m[Z // 3, Y // 3, :] = True
    for a in range(3):
        assert m.take(0, axis=a).any() and m.take(-1, axis=a).any()
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_segment_meshes_match_the_restatement_bit_for_bit(volumes, layout):
    g = volumes["noise"]
    r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        d = densities("noise", g, r.bind_uniforms())
        lo = float(np.quantile(d, 0.7))
        z, y, x = np.unravel_index(int(np.argmax(d)), d.shape)
        s = r.segment((int(x), int(y), int(z)), lo, connectivity=26)
        assert s.count > 100
        stages = [("segment", lambda: None), ("closed", lambda: r.segment_edit("close", steps=2, connectivity=6)),
                  ("uploaded", lambda: r.set_segment_mask(_touching_all_faces(d.shape)))]
        for stage, act in stages:
            act()
            mask = r.segment_mask()
            for name, box in BOXES.items():
                got = _raw(r, segment=True, box=box)
                _same(got, MR.extract_segment(mask, box), (layout, stage, name))
                _same_result(r.last_mesh_result, mask, box)
                again = _raw(r, segment=True, box=box)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))
            assert np.array_equal(r.segment_mask(), mask)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("vol", ["serpentine", "tube"])
def test_thin_and_long_volumes(volumes, vol):
    g = volumes[vol]
    r = renderer(g, dvr_jitter=False)
    try:
        d = densities(vol, g, r.bind_uniforms())
        iso = float(d.max()) / 2
        _same(_raw(r, iso=iso), MR.extract_density(d, iso), vol)
        _same_result(r.last_mesh_result, d >= F32(iso), None)
    finally:
        r.close()


@pytest.mark.gpu
def test_every_layout_returns_the_same_raw_arrays_and_the_launch_count_is_constant(volumes):
    g = volumes["phantom"]
    raws, launches = {}, set()
    for layout in sorted(LAYOUTS):
        r = renderer(g, layout=LAYOUTS[layout], dvr_jitter=False)
        try:
            d = densities("phantom", g, r.bind_uniforms())
            out = []
            for iso in (0.75, 0.3, float(d.max()) * 2):
                out.append(_raw(r, iso=iso))
                launches.add(r.mesh_stats()[0])
            r.segment((32, 32, 32), 0.0, connectivity=6)
            out.append(_raw(r, segment=True))
            launches.add(r.mesh_stats()[0])
            assert all(ms >= 0 for ms in r.mesh_stats()[1:])
            raws[layout] = b"".join(a.tobytes() for o in out for a in o)
            assert len({len(o[0]) for o in out}) > 2   # meshes of different sizes, one of them empty
        finally:
            r.close()
    assert len(set(raws.values())) == 1
    assert len(launches) == 1


@pytest.mark.gpu
def test_rendering_the_segment_its_view_and_pick_are_left_alone(volumes):
    g = volumes["phantom"]
    r = renderer(g, dvr_jitter=False)
    try:
        r.bind_uniforms()
        s0 = r.segment((32, 32, 32), 0.3, connectivity=26)
        assert s0.count > 0
        dense_off = _raw(r, iso=0.5)
        r.reset_counters()
        r.restart_rendering()
        r.render(frames=2, in_flight=1)
        a = r.read_accum().copy()
        c1 = r.counters()
        c1 = {f: getattr(c1, f) for f, _ in c1._fields_}
        frame = r.frame_index
        st, m = r.segment_stats(), r.segment_mask()
        for kw in ({"iso": 0.75}, {"segment": True}, {"iso": 0.2, "box": ((0, 0, 0), (31, 63, 63))}, {"iso": 1e9}):
            r.extract_mesh(**kw)
        b = r.read_accum().copy()
        c2 = r.counters()
        c2 = {f: getattr(c2, f) for f, _ in c2._fields_}
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
        assert c1 == c2 and frame == r.frame_index == 2
        assert r.segment_stats() == st and np.array_equal(r.segment_mask(), m)
        r.render(frames=1, in_flight=1)
        assert r.counters().frames == c1["frames"] + 1 and r.frame_index == 3
        # the view and pick
        r.segment_view = "hide"
        w, h = r.width, r.height
        pick = r.pick(w // 2, h // 2, 0.5)
        dense_hide = _raw(r, iso=0.5)
        assert r.segment_view == "hide"
        assert r.pick(w // 2, h // 2, 0.5) == pick
        assert all(x.tobytes() == y.tobytes() for x, y in zip(dense_off, dense_hide))
        assert np.array_equal(r.segment_mask(), m)
    finally:
        r.close()


@pytest.mark.gpu
def test_refusals_limits_and_staleness(volumes):
    from volxel_amd import _abi
    g = volumes["noise"]
    lib = _abi.load_library()
    q = _abi.VxMeshParams()
    q.source, q.iso = 0, 0.3
    for a in range(3):
        q.box_lo[a], q.box_hi[a] = 0, 0xffffffff
    res = _abi.VxMeshResult()
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0

    def refused(code, word, fn=None):
        rc = fn() if fn else lib.vx_mesh_extract(ctx, C.byref(q), C.byref(res))
        msg = lib.vx_last_error(ctx).decode()
        assert rc == code and word in msg, (rc, msg)

    try:
        refused(3, "no volume")
        assert upload_volume(lib, ctx, g) == 0
        refused(1, "vx_set_params")
        r = renderer(g, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_set_params(ctx, C.byref(p)) == 0
        refused(1, "params is NULL", lambda: lib.vx_mesh_extract(ctx, None, C.byref(res)))
        refused(1, "no current mesh", lambda: lib.vx_mesh_read(ctx, None, None, None))
        q.source = 2
        refused(1, "source")
        q.source = 0
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            q.iso = bad
            refused(1, "iso")
        q.iso = 0.3
        q.box_lo[1], q.box_hi[1] = 9, 8
        refused(1, "box axis 1")
        q.box_lo[1], q.box_hi[1] = 0, 64
        refused(1, "box axis 1")
        q.box_hi[1] = 0xffffffff
        q.source = 1
        refused(1, "no current segment")
        q.source = 0
        assert lib.vx_mesh_extract(ctx, C.byref(q), C.byref(res)) == 0 and res.vertices > 0 and res.triangles > 0
        nv, nt = int(res.vertices), int(res.triangles)
        assert lib.vx_mesh_read(ctx, None, None, None) == 0
        # a refused call leaves the mesh
        q.iso = -1.0
        refused(1, "iso")
        v = np.zeros((nv, 3), F32)
        assert lib.vx_mesh_read(ctx, v.ctypes.data_as(C.c_void_p), None, None) == 0 and np.isfinite(v).all()
        q.iso = 0.3
        # the limits: the message carries both counts, and no mesh is kept
        q.max_vertices = nv - 1
        refused(1, f"{nv} vertices and {nt} triangles")
        refused(1, "no current mesh", lambda: lib.vx_mesh_read(ctx, None, None, None))
        q.max_vertices, q.max_triangles = nv, nt - 1
        refused(1, "max_triangles")
        q.max_triangles = nt
        assert lib.vx_mesh_extract(ctx, C.byref(q), None) == 0
        assert lib.vx_mesh_read(ctx, None, None, None) == 0
        # an upload drops the mesh
        assert upload_volume(lib, ctx, g) == 0
        refused(1, "no current mesh", lambda: lib.vx_mesh_read(ctx, None, None, None))
        assert lib.vx_mesh_extract(ctx, C.byref(q), C.byref(res)) == 0 and (int(res.vertices), int(res.triangles)) == (nv, nt)
    finally:
        lib.vx_destroy(ctx)


@pytest.mark.gpu
def test_python_refusals_on_a_live_renderer(volumes):
    r = renderer(volumes["noise"], dvr_jitter=False)
    try:
        with pytest.raises(ValueError, match="box"):
            r.extract_mesh(0.3, box=((0, 0, 0), (64, 5, 5)))
        from volxel_amd import VolxelError
        with pytest.raises(VolxelError, match="no current segment"):
            r.extract_mesh(segment=True)
        with pytest.raises(VolxelError, match="max_vertices"):
            r.extract_mesh(0.3, max_vertices=10)
    finally:
        r.close()


@pytest.mark.gpu
def test_device_group_runs_the_mesher_on_member0(volumes):
    g = volumes["noise"]
    one = renderer(g, dvr_jitter=False)
    try:
        want = _raw(one, iso=0.3)
        one.segment((10, 10, 10), 0.2, connectivity=26)
        want_s = _raw(one, segment=True)
    finally:
        one.close()
    grp = renderer(g, devices=[0, 0], dvr_jitter=False)
    try:
        got = _raw(grp, iso=0.3)
        grp.segment((10, 10, 10), 0.2, connectivity=26)
        got_s = _raw(grp, segment=True)
        assert grp.mesh_stats()[0] > 0
    finally:
        grp.close()
    assert all(a.tobytes() == b.tobytes() for a, b in zip(want + want_s, got + got_s))


def _ball(n=64):
    z, y, x = np.meshgrid(*[np.arange(n)] * 3, indexing="ij")
    c = (n - 1) / 2
    r = np.sqrt((x - c) ** 2 + (y - c) ** 2 + (z - c) ** 2)
    v = np.clip(4000.0 * (1.0 - r / n), 0, 4095)
    return v.astype(np.uint16), (1.0, 1.0, 1.0)


@pytest.mark.gpu
def test_world_space_agrees_with_voxel_index_and_pick():
    g = grid(*_ball())
    r = renderer(g, size=(96, 96), dvr_jitter=False)
    try:
        d = SG.densities(g, r.bind_uniforms().volume_density_scale, r.bind_uniforms().volume_inv_maj)
        iso = float(d.max()) * 0.75
        mv = r.extract_mesh(iso, space="voxel")
        mw = r.extract_mesh(iso, space="world")
        mg = r.extract_mesh(iso, space="grid")
        assert len(mw.vertices) == len(mv.vertices) > 1000
        assert mv.volume() > 0 and mw.volume() > 0 and mg.volume() > 0
        for k in range(0, len(mw.vertices), 37):
            i = r.voxel_index(mw.vertices[k])
            assert i is not None and all(abs(a - (c + 0.5)) <= 1.0 for a, c in zip(i, mv.cells[k])), (i, mv.cells[k])
        # one voxel's world diagonal
        t = np.asarray(r.volume.combined_transform(), dtype=np.float64)[:3, :3]
        diag = float(np.linalg.norm(t @ np.ones(3)))
        hits = 0
        for px in range(8, 96, 8):
            for py in range(8, 96, 8):
                w = r.pick(px, py, iso)
                if w is None:
                    continue
                hits += 1
                dist = float(np.min(np.linalg.norm(mw.vertices - np.asarray(w), axis=1)))
                assert dist <= diag, (px, py, dist, diag)
        assert hits > 10
    finally:
        r.close()


@pytest.mark.gpu
def test_js_host_has_the_python_arrays_and_stl_bytes(volumes, tmp_path):
    g = volumes["noise"]
    box = ((2, 3, 4), (50, 60, 61))
    r = renderer(g, dvr_jitter=False)
    try:
        m = r.extract_mesh(0.3, space="voxel", box=box)
        m.write_stl(tmp_path / "py.stl")
        r.segment((10, 10, 10), 0.2, connectivity=26)
        s = r.extract_mesh(segment=True, space="world")
        launches = r.mesh_stats()[0]
    finally:
        r.close()
    dump_grid(tmp_path, g)
    body = r"""
const m = r.extractMesh({ iso: 0.3, space: 'voxel', box: [[2, 3, 4], [50, 60, 61]] });
save('v.bin', m.vertices); save('c.bin', m.cells); save('t.bin', m.triangles);
fs.writeFileSync(path.join(dir, 'js.stl'), r.meshToStl(m));
r.segment([10, 10, 10], 0.2, { connectivity: 26 });
const s = r.extractMesh({ segment: true });
save('sv.bin', s.vertices); save('st.bin', s.triangles);
let refused = '';
try { r.extractMesh({ iso: 0.3, maxVertices: 10 }); } catch (e) { refused = String(e.message); }
let both = '';
try { r.extractMesh({ iso: 0.3, segment: true }); } catch (e) { both = String(e.message); }
console.log(JSON.stringify({ st: r.meshStats(), refused, both }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert np.array_equal(np.fromfile(tmp_path / "v.bin", dtype=np.float64).reshape(-1, 3), m.vertices)
    assert np.array_equal(np.fromfile(tmp_path / "c.bin", dtype=np.int32).reshape(-1, 3), m.cells)
    assert np.array_equal(np.fromfile(tmp_path / "t.bin", dtype=np.uint32).reshape(-1, 3), m.triangles)
    assert len(m.triangles) > 1000
    assert (tmp_path / "js.stl").read_bytes() == (tmp_path / "py.stl").read_bytes()
    assert np.array_equal(np.fromfile(tmp_path / "st.bin", dtype=np.uint32).reshape(-1, 3), s.triangles)
    js_world = np.fromfile(tmp_path / "sv.bin", dtype=np.float64).reshape(-1, 3)
    assert js_world.shape == s.vertices.shape and np.allclose(js_world, s.vertices, rtol=0, atol=1e-12)
    assert "max_vertices" in out["refused"] and "exactly one" in out["both"] and out["st"]["launches"] == launches
