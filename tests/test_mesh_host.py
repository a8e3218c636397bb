"""The mesher's contract on the CPU (DESIGN.md section 2 "Meshes"): the NumPy restatement (tests/mesh_ref.py) against things it
cannot have copied -- invariants that hold for every input, the topology of closed forms, float64 closed-form geometry,
negative controls that must each fail a check, the STL / PLY writers parsed back, the refusals that need no GPU and the surface
of the C ABI and the JS typings.

Measured with this restatement (ball of radius 0.3 N, linear radial field, relative errors against 4/3 pi R^3 and 4 pi R^2):
    N              32          64          128
    density volume -1.2397 %   -0.3105 %   -0.0776 %     (ratios 3.99, 4.00: second order)
    density area   -0.6750 %   -0.1652 %   -0.0415 %     (ratios 4.09, 3.98)
    segment volume -2.6843 %   -0.9019 %   -0.1542 %     (midpoint crossings; the voxel count itself is off by -1.56 % / -0.62 % /
                                                          -0.084 %)
An all-inside 8^3 volume meshes to a volume of 489.875 (the cap sits half a voxel out, edges and corners cut)."""
import ctypes as C
import os
import struct

import numpy as np
import pytest

from tests import mesh_ref as MR
from tests.common import F32, ROOT
from tests.shapes import odd
BALL_VOLUME_ERR = {32: 0.012397, 64: 0.003105, 128: 0.000776}
BALL_AREA_ERR = {32: 0.006750, 64: 0.001652, 128: 0.000415}
SEGMENT_VOLUME_ERR = {32: 0.026843, 64: 0.009019, 128: 0.001542}


def _radius(n, centre=None):
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    cx, cy, cz = centre if centre is not None else ((n - 1) / 2,) * 3
    return np.sqrt((x - cx) ** 2 + (y - cy) ** 2 + (z - cz) ** 2)


def _ball_field(n):
    """linear in the radius: the surface f = iso is the sphere of radius 0.3 n"""
    return (1.0 - _radius(n) / n).astype(F32), F32(1.0 - 0.3)


def _noise(n, seed):
    return np.random.default_rng(seed).random((n, n, n)).astype(F32)


def _phantom():
    from volxel_amd import synth
    v, _ = synth.ct_phantom(64)
    return (v.astype(F32) / F32(4095)).astype(F32)


def _odd_field():
    v, _ = odd()
    out = np.zeros((48, 32, 40), dtype=F32)
    out[:45, :29, :37] = v.astype(F32) / F32(4095)
    return out


def _inputs():
    """(name, inside, f, iso, box) over both sources, with and without a box"""
    out = []
    for n, seed in ((24, 1), (40, 2), (64, 3)):
        f = _noise(n, seed)
        out.append((f"noise{n}", f >= F32(0.55), f, 0.55, None))
        out.append((f"noise{n}_box", f >= F32(0.4), f, 0.4, ((3, 0, 5), (n - 4, n - 1, n - 2))))
        m = f >= F32(0.6)
        out.append((f"noise{n}_segment", m, m.astype(F32), 0.5, None))
    ph = _phantom()
    out.append(("phantom", ph >= F32(0.3), ph, 0.3, None))
    out.append(("phantom_box", ph >= F32(0.2), ph, 0.2, ((8, 16, 0), (39, 47, 63))))
    od = _odd_field()
    q = float(np.quantile(od[od > 0], 0.5))
    out.append(("odd", od >= F32(q), od, q, None))
    m = od >= F32(q)
    out.append(("odd_segment_box", m, m.astype(F32), 0.5, ((0, 0, 0), (20, 31, 47))))
    ones = np.ones((16, 8, 24), dtype=bool)
    out.append(("all_inside", ones, ones.astype(F32), 0.5, None))
    out.append(("all_inside_box", ones, ones.astype(F32), 0.5, ((1, 1, 1), (6, 6, 6))))
    return out


def _check_invariants(inside, f, iso, box, **kw):
    """the checks every extracted mesh passes; returns the names of those that fail"""
    v, c, t = MR.extract(inside, f, iso, box, **kw)
    want = MR.counts(inside, box)
    bad = []
    if not MR.closed_and_oriented(t):
        bad.append("closed")
    if len(t) and not MR.volume(v, t) > 0:
        bad.append("volume")
    if not ((c.astype(F32) <= v).all() and (v <= (c + 1).astype(F32)).all()):
        bad.append("within_cell")
    if len(v) != want["vertices"] or len(np.unique(c, axis=0)) != len(c):
        bad.append("vertices")
    if len(t) != want["triangles"]:
        bad.append("triangles")
    if len(t) and ((t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])).any():
        bad.append("repeated_index")
    return bad


@pytest.mark.parametrize("case", _inputs(), ids=lambda c: c[0])
def test_invariants_hold_for_every_input(case):
    _, inside, f, iso, box = case
    assert _check_invariants(inside, f, iso, box) == []
    v, c, t = MR.extract(inside, f, iso, box)
    e = MR.directed_edges(t)
    n = int(e.max()) + 1
    most = int(np.unique(e[:, 0] * n + e[:, 1], return_counts=True)[1].max())
    # at an ambiguous face four triangles share an edge: "every edge exactly twice" is not the condition, and noise shows it
    assert most == 2 if "noise" in case[0] else most in (1, 2)
    cv, cc, ct = MR.canonical(v, c, t)
    assert np.array_equal(cv, v) and np.array_equal(cc, c) and len(ct) == len(t)   # the restatement emits (z, y, x) order
    rng = np.random.default_rng(0)   # canonical() undoes a relabelling, a rotation of each triangle and a shuffle
    perm = rng.permutation(len(v))
    inv = np.argsort(perm)
    t2 = inv[t.astype(np.int64)]
    t2 = np.stack([np.roll(r, k) for r, k in zip(t2, rng.integers(0, 3, len(t2)))]) if len(t2) else t2
    sv, sc, st = MR.canonical(v[perm], c[perm], t2[rng.permutation(len(t2))] if len(t2) else t2)
    assert np.array_equal(sv, cv) and np.array_equal(sc, cc) and np.array_equal(st, ct)


def test_topology_of_closed_forms():
    n = 40
    ball = _radius(n) <= 12.3
    v, _, t = MR.extract_segment(ball)
    assert MR.euler(len(v), t) == 2
    z, y, x = np.meshgrid(*[np.arange(n, dtype=np.float64)] * 3, indexing="ij")
    c = (n - 1) / 2
    torus = (np.sqrt((x - c) ** 2 + (y - c) ** 2) - 11.0) ** 2 + (z - c) ** 2 <= 4.2 ** 2
    v, _, t = MR.extract_segment(torus)
    assert MR.euler(len(v), t) == 0
    f = (1.0 - np.sqrt((np.sqrt((x - c) ** 2 + (y - c) ** 2) - 11.0) ** 2 + (z - c) ** 2) / n).astype(F32)
    v, _, t = MR.extract_density(f, 1.0 - 4.2 / n)
    assert MR.euler(len(v), t) == 0
    two = (_radius(n, (10, 10, 10)) <= 6.4) | (_radius(n, (28, 27, 29)) <= 7.7)
    v, _, t = MR.extract_segment(two)
    assert MR.euler(len(v), t) == 4
    ones = np.ones((8, 8, 8), dtype=bool)
    v, _, t = MR.extract_segment(ones)
    assert MR.euler(len(v), t) == 2
    assert 7 ** 3 < MR.volume(v, t) < 8 ** 3
    assert abs(MR.volume(v, t) - 489.875) < 1e-6


def test_ball_geometry_converges_at_second_order():
    """density: the ratios of successive errors lie in [3, 5] and N = 64 is within twice its measured error; segment: the error
    shrinks from 32 to 64 to 128 and each is within twice its measured value (the module docstring holds the figures)"""
    ev, ea, es = {}, {}, {}
    for n in (32, 64, 128):
        R = 0.3 * n
        V, A = 4.0 / 3.0 * np.pi * R ** 3, 4.0 * np.pi * R ** 2
        f, iso = _ball_field(n)
        v, _, t = MR.extract_density(f, iso)
        ev[n], ea[n] = abs(MR.volume(v, t) / V - 1), abs(MR.area(v, t) / A - 1)
        v, _, t = MR.extract_segment(f >= iso)
        es[n] = abs(MR.volume(v, t) / V - 1)
        print(n, ev[n], ea[n], es[n])
    for e in (ev, ea):
        assert 3 <= e[32] / e[64] <= 5 and 3 <= e[64] / e[128] <= 5, e
    assert ev[64] <= 2 * BALL_VOLUME_ERR[64] and ea[64] <= 2 * BALL_AREA_ERR[64]
    assert es[32] > es[64] > es[128]
    for n in es:
        assert es[n] <= 2 * SEGMENT_VOLUME_ERR[n], (n, es[n])


def _geometry_ok(**kw):
    f, iso = _ball_field(32)
    R = 0.3 * 32
    v, _, t = MR.extract(f >= iso, f, iso, **kw)
    return (abs(MR.volume(v, t) / (4.0 / 3.0 * np.pi * R ** 3) - 1) <= 2 * BALL_VOLUME_ERR[32] and
            abs(MR.area(v, t) / (4.0 * np.pi * R ** 2) - 1) <= 2 * BALL_AREA_ERR[32])


def test_negative_controls_each_fail_a_check():
    f = _noise(24, 7)
    inside = f >= F32(0.5)
    assert _check_invariants(inside, f, 0.5, None) == [] and _geometry_ok()
    # no outside rule: the mesh is open where the structure meets the faces of the volume
    assert "closed" in _check_invariants(inside, f, 0.5, None, no_outside=True)
    ones = np.ones((8, 8, 8), dtype=bool)
    assert len(MR.extract(ones, ones.astype(F32), 0.5, no_outside=True)[2]) == 0
    # unflipped winding: not consistently oriented
    assert "closed" in _check_invariants(inside, f, 0.5, None, unflipped=True)
    # t measured from the wrong end, and the mean over 12 instead of n: still closed, wrong geometry
    assert _check_invariants(inside, f, 0.5, None, t_from_far_end=True) == []
    assert not _geometry_ok(t_from_far_end=True)
    assert not _geometry_ok(n12=True)


def _mesh(space="voxel"):
    from volxel_amd import Mesh
    f = _noise(24, 5)
    v, c, t = MR.extract_density(f, 0.5)
    return Mesh(v.astype(np.float64), c, t, space)


def test_measures_and_mirroring():
    m = _mesh()
    assert m.volume() == pytest.approx(MR.volume(m.vertices, m.triangles)) and m.volume() > 0
    assert m.area() == pytest.approx(MR.area(m.vertices, m.triangles))
    scale = np.diag([2.0, 3.0, 0.5, 1.0])
    scale[:3, 3] = (1, -2, 3)
    s = m.transformed(scale, "grid")
    assert s.volume() == pytest.approx(3.0 * m.volume()) and np.array_equal(s.triangles, m.triangles) and s.space == "grid"
    mirror = np.diag([-1.0, 1.0, 1.0, 1.0])
    r = m.transformed(mirror, "world")
    assert r.volume() == pytest.approx(m.volume()) and r.volume() > 0
    assert np.array_equal(r.triangles, m.triangles[:, [0, 2, 1]])


def test_stl_round_trip(tmp_path):
    m = _mesh()
    m.triangles = np.concatenate([m.triangles, np.array([[0, 0, 1]], dtype=np.uint32)])   # a degenerate triangle
    path = tmp_path / "m.stl"
    m.write_stl(path)
    raw = path.read_bytes()
    M = len(m.triangles)
    assert len(raw) == 84 + 50 * M and struct.unpack("<I", raw[80:84])[0] == M
    rec = np.frombuffer(raw[84:], dtype=np.dtype([("n", "<f4", 3), ("v", "<f4", (3, 3)), ("a", "<u2")]))
    want = m.vertices.astype(F32)[m.triangles.astype(np.int64)]
    assert np.array_equal(rec["v"], want) and not rec["a"].any()
    n = np.cross(want[:, 1].astype(np.float64) - want[:, 0], want[:, 2].astype(np.float64) - want[:, 0])
    ln = np.linalg.norm(n, axis=1)
    assert ln[-1] == 0 and np.array_equal(rec["n"][-1], np.zeros(3, F32))
    assert np.allclose(rec["n"][:-1], n[:-1] / ln[:-1, None], atol=1e-6)
    assert np.allclose(np.linalg.norm(rec["n"][:-1].astype(np.float64), axis=1), 1.0, atol=1e-6)


def test_ply_round_trip(tmp_path):
    m = _mesh()
    path = tmp_path / "m.ply"
    m.write_ply(path)
    raw = path.read_bytes()
    N, M = len(m.vertices), len(m.triangles)
    head = (f"ply\nformat binary_little_endian 1.0\ncomment volxel_amd\nelement vertex {N}\nproperty float x\nproperty float y\n"
            f"property float z\nelement face {M}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")
    assert raw.startswith(head) and len(raw) == len(head) + 12 * N + 13 * M
    body = raw[len(head):]
    assert np.array_equal(np.frombuffer(body[:12 * N], dtype="<f4").reshape(N, 3), m.vertices.astype(F32))
    faces = np.frombuffer(body[12 * N:], dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
    assert (faces["n"] == 3).all() and np.array_equal(faces["i"], m.triangles.astype(np.int32))


def test_extract_mesh_refusals_that_need_no_gpu():
    from volxel_amd import Volxel3DRenderer
    from volxel_amd.mesh import check_extract_args
    for kw in ({}, {"iso": 0.5, "segment": True}):
        with pytest.raises(ValueError, match="exactly one"):
            check_extract_args(kw.get("iso"), kw.get("segment", False), "world", 0, 0)
    for iso in (0.0, -1.0, float("nan"), float("inf"), 1e39):
        with pytest.raises(ValueError, match="iso"):
            check_extract_args(iso, False, "world", 0, 0)
    with pytest.raises(ValueError, match="space"):
        check_extract_args(0.5, False, "mm", 0, 0)
    with pytest.raises(ValueError, match="segment"):
        check_extract_args(None, 1, "world", 0, 0)
    for bad in (-1, 2 ** 32, 1.5, True):
        with pytest.raises(ValueError, match="max_vertices"):
            check_extract_args(0.5, False, "world", bad, 0)
        with pytest.raises(ValueError, match="max_triangles"):
            check_extract_args(0.5, False, "world", 0, bad)
    assert check_extract_args(0.5, False, "voxel", 0, 7) == F32(0.5) and check_extract_args(None, True, "grid", 1, 0) is None
    assert callable(Volxel3DRenderer.extract_mesh) and callable(Volxel3DRenderer.mesh_stats)


def test_surface_of_the_abi_and_the_typings():
    from volxel_amd import _abi
    names = _abi.declared_symbols("volxel_hip.h")
    assert {"vx_mesh_extract", "vx_mesh_read", "vx_mesh_stats"} <= set(names)
    P = _abi.VxMeshParams
    assert C.sizeof(P) == 40
    assert [(n, getattr(P, n).offset) for n, _ in P._fields_] == [("source", 0), ("iso", 4), ("box_lo", 8), ("box_hi", 20),
                                                                 ("max_vertices", 32), ("max_triangles", 36)]
    R = _abi.VxMeshResult
    assert C.sizeof(R) == 56 and R.blocks.offset == 24 and R.bbox_lo.offset == 32 and R.bbox_hi.offset == 44
    assert (_abi.MESH_DENSITY, _abi.MESH_SEGMENT) == (0, 1)
    header = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    assert "VX_MESH_DENSITY = 0" in header and "VX_MESH_SEGMENT = 1" in header
    dts = open(os.path.join(ROOT, "volxel_amd", "napi", "index.d.ts")).read()
    for name in ("extractMesh(", "meshStats(", "meshToStl("):
        assert name in dts
    js = open(os.path.join(ROOT, "volxel_amd", "napi", "viewer.js")).read()
    shim = open(os.path.join(ROOT, "volxel_amd", "napi", "volxel_napi.c")).read()
    assert "extractMesh(" in js and "meshToStl(" in js and "vx_mesh_extract(" in shim and "vx_mesh_read(" in shim


def test_library_exports_the_mesher(native_lib):
    for name in ("vx_mesh_extract", "vx_mesh_read", "vx_mesh_stats"):
        assert getattr(native_lib, name) is not None
