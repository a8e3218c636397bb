"""The mesher of `Volxel3DRenderer` (vx_api_mesh.hip); the meshes themselves are volxel_amd.mesh.  A mixin: the renderer
supplies _lib, _ctx, _check, _out, _index_extent and bind_uniforms."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _checks
from .mesh import Mesh, check_extract_args


class MeshMixin:
    def extract_mesh(self, iso=None, *, segment: bool = False, box=None, space: str = "world", max_vertices: int = 0,
                     max_triangles: int = 0) -> Mesh:
        """The surface of the isosurface d = iso, or (segment=True) of the current segment, as a closed, indexed triangle mesh
        (vx_mesh_extract, DESIGN.md section 2 "Meshes": naive surface nets on the GPU).  Exactly one of iso / segment=True.
        box = ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices, or None for the whole volume; voxels outside it (and
        outside the volume) count as outside, so the mesh is capped there.  space: "voxel" (voxel i at i, the device's
        coordinates), "grid" (grid.transform * (q + 1/2, 1): mm for DICOM, the space of Segment.volume_grid) or "world" (the
        space of pick()).  max_vertices / max_triangles: refuse a larger mesh (0: 2^32 - 2).  Binds the current uniforms."""
        iso32 = check_extract_args(iso, segment, space, max_vertices, max_triangles)
        q = _abi.VxMeshParams()
        q.box_lo[:], q.box_hi[:] = _checks.box(box, self._index_extent("extract_mesh"))
        q.source = _abi.MESH_SEGMENT if segment else _abi.MESH_DENSITY
        q.iso = 0.0 if segment else float(iso32)
        q.max_vertices, q.max_triangles = int(max_vertices), int(max_triangles)
        self.bind_uniforms()
        res = _abi.VxMeshResult()
        self._check(self._lib.vx_mesh_extract(self._ctx, C.byref(q), C.byref(res)))
        self.last_mesh_result = res
        nv, nt = int(res.vertices), int(res.triangles)
        verts = np.empty((nv, 3), dtype=np.float32)
        cells = np.empty((nv, 3), dtype=np.int32)
        tris = np.empty((nt, 3), dtype=np.uint32)
        self._check(self._lib.vx_mesh_read(self._ctx, verts.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                                           tris.ctypes.data_as(C.c_void_p)))
        mesh = Mesh(verts.astype(np.float64), cells, tris, "voxel")
        if space == "voxel":
            return mesh
        half = np.eye(4)
        half[:3, 3] = 0.5   # voxel i occupies [i, i + 1] in index space
        m = np.asarray(self.volume.grid.transform if space == "grid" else self.volume.combined_transform(), dtype=np.float64)
        return mesh.transformed(m @ half, space)

    def mesh_stats(self):
        """(launches, inside_ms, active_and_scan_ms, emit_ms) of the last extract_mesh (vx_mesh_stats)"""
        return self._out("vx_mesh_stats", C.c_uint32, C.c_double * 3)
