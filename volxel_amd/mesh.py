"""Triangle meshes from the GPU mesher (Volxel3DRenderer.extract_mesh, DESIGN.md section 2 "Meshes"): the arrays, their
measures in float64, and binary STL / PLY writers.  Pure NumPy: nothing here touches the device."""
from __future__ import annotations

import struct
from dataclasses import dataclass

import numpy as np

from . import _checks

MESH_SPACES = ("voxel", "grid", "world")


@dataclass
class Mesh:
    """vertices (N, 3) float64 in `space`, cells (N, 3) int32 (each vertex's grid cell, components >= -1), triangles (M, 3)
    uint32 wound so that normals point out of the structure"""
    vertices: np.ndarray
    cells: np.ndarray
    triangles: np.ndarray
    space: str = "voxel"

    def _corners(self):
        t = self.triangles.astype(np.int64)
        v = np.asarray(self.vertices, dtype=np.float64)
        return v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]

    def area(self) -> float:
        """the sum of half the cross-product norms"""
        a, b, c = self._corners()
        return float(0.5 * np.linalg.norm(np.cross(b - a, c - a), axis=1).sum())

    def volume(self) -> float:
        """the signed volume, sum of a . (b x c) / 6: positive for every extracted mesh"""
        a, b, c = self._corners()
        return float(np.einsum("ij,ij->i", a, np.cross(b, c)).sum() / 6.0)

    def transformed(self, matrix4, space: str) -> "Mesh":
        """the mesh under a 4 x 4 affine map (float64); a mirroring map swaps two indices of every triangle, so that volume()
        stays positive"""
        m = np.asarray(matrix4, dtype=np.float64).reshape(4, 4)
        v = np.asarray(self.vertices, dtype=np.float64) @ m[:3, :3].T + m[:3, 3]
        t = self.triangles
        if np.linalg.det(m[:3, :3]) < 0:
            t = np.ascontiguousarray(t[:, [0, 2, 1]])
        return Mesh(v, self.cells, t, space)

    def stl_bytes(self) -> bytes:
        """binary STL: an 80-byte header, the u32 triangle count, 50 bytes per triangle (the unit facet normal of the float32
        corners -- (0, 0, 0) for a degenerate triangle --, three float32 corners, a zero attribute word)"""
        a, b, c = (x.astype(np.float32) for x in self._corners())
        # in float64 from the float32 corners, every product and sum spelled out (the JS host's meshToStl does the same)
        u, w = b.astype(np.float64) - a.astype(np.float64), c.astype(np.float64) - a.astype(np.float64)
        n = np.stack([u[:, 1] * w[:, 2] - u[:, 2] * w[:, 1], u[:, 2] * w[:, 0] - u[:, 0] * w[:, 2],
                      u[:, 0] * w[:, 1] - u[:, 1] * w[:, 0]], axis=1)
        ln = np.sqrt(n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1] + n[:, 2] * n[:, 2])
        ok = ln > 0
        n[ok] /= ln[ok, None]
        n[~ok] = 0.0
        rec = np.zeros(len(a), dtype=np.dtype([("n", "<f4", 3), ("a", "<f4", 3), ("b", "<f4", 3), ("c", "<f4", 3), ("attr", "<u2")]))
        rec["n"], rec["a"], rec["b"], rec["c"] = n.astype(np.float32), a, b, c
        head = b"volxel_amd binary STL".ljust(80, b" ")
        return head + struct.pack("<I", len(a)) + rec.tobytes()

    def write_stl(self, path) -> None:
        with open(path, "wb") as f:
            f.write(self.stl_bytes())

    def ply_header(self) -> bytes:
        return ("ply\nformat binary_little_endian 1.0\ncomment volxel_amd\n"
                f"element vertex {len(self.vertices)}\nproperty float x\nproperty float y\nproperty float z\n"
                f"element face {len(self.triangles)}\nproperty list uchar int vertex_indices\nend_header\n").encode("ascii")

    def write_ply(self, path) -> None:
        """binary little-endian PLY: float vertices, uchar-counted int faces"""
        face = np.zeros(len(self.triangles), dtype=np.dtype([("n", "u1"), ("i", "<i4", 3)]))
        face["n"] = 3
        face["i"] = self.triangles.astype(np.int64)
        with open(path, "wb") as f:
            f.write(self.ply_header())
            f.write(np.asarray(self.vertices, dtype="<f4").tobytes())
            f.write(face.tobytes())


def check_extract_args(iso, segment, space, max_vertices, max_triangles):
    """the refusals of extract_mesh that need no device; returns iso as float32 (None for a segment)"""
    if not isinstance(segment, bool):
        raise ValueError(f"segment must be True or False, not {segment!r}")
    if (iso is None) == (not segment):
        raise ValueError("extract_mesh takes exactly one of iso and segment=True")
    if space not in MESH_SPACES:
        raise ValueError(f"space must be one of {MESH_SPACES}, not {space!r}")
    for name, v in (("max_vertices", max_vertices), ("max_triangles", max_triangles)):
        _checks.integer(v, 0, 2 ** 32 - 1, f"{name} must be an integer 0 .. 2^32 - 1, not {v!r}")
    if segment:
        return None
    with np.errstate(over="ignore"):
        iso32 = np.float32(iso)
    if not (np.isfinite(iso32) and iso32 > 0):
        raise ValueError(f"iso must be finite and > 0, not {iso!r}")
    return iso32
