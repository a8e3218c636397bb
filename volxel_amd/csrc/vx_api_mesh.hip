// vx_api_mesh.hip -- the mesh unit of the host layer (units: DESIGN.md section 4.1): surface meshes of isosurfaces and of
// the current segment (vx_mesh_extract, vx_mesh_read).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "vx_mesh.hpp"
#include "vx_context.hpp"

using namespace vx;

namespace {

// ---- meshes (vx_mesh_extract, vx_mesh_read; kernels in vx_mesh.hpp) -----------------------------------------------------------
// Five launches whatever the mesh: the inside words, the active cells with their counts, the two launches that finish the
// exclusive scan, the emission.  The totals are read back once, between the scan and the emission, to size the outputs.
static int ensure_mesh(VxContext* c) {
  if (c->vol.mesh_alloc) return VX_OK;
  MeshDev& m = c->vol.mesh;
  for (int a = 0; a < 3; ++a) {
    m.bc[a] = c->vol.dv.bc[a];
    m.cb[a] = c->vol.dv.bc[a] + 1u;
  }
  const size_t nb = (size_t)m.bc[0] * m.bc[1] * m.bc[2], ncb = (size_t)m.cb[0] * m.cb[1] * m.cb[2];
  if (ncb > 0xffffff00ull) VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_extract: %zu cell blocks are beyond the 32-bit block index", ncb);
  const size_t np = (ncb + 255u) / 256u;
  const int rc = carve(c, c->vol.mesh_alloc, [&](Carve& k) {
    m.inside = k.take<uint64_t>(nb * 8u);
    m.act = k.take<uint64_t>(ncb * 8u);
    m.vq = k.take<uint2>(ncb);
    m.off = k.take<uint2>(ncb);
    m.part = k.take<uint2>(np);
    m.poff = k.take<uint2>(np);
    m.st = k.take<MeshStats>();
  });
  if (rc) return rc;
  m.nb = (uint32_t)nb;
  m.ncb = (uint32_t)ncb;
  m.np = (uint32_t)np;
  return VX_OK;
}

}  // namespace

extern "C" {

int vx_mesh_extract(VxContext* c, const VxMeshParams* mp, VxMeshResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_mesh_extract(c->members[0], mp, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_mesh_extract", mp, "params")) return rc;
  if (mp->source != VX_MESH_DENSITY && mp->source != VX_MESH_SEGMENT)
    VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_extract: source = %d is not VX_MESH_DENSITY or VX_MESH_SEGMENT", mp->source);
  const bool segment = mp->source == VX_MESH_SEGMENT;
  if (!segment && !(std::isfinite(mp->iso) && mp->iso > 0.0f))
    VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_extract: iso = %g is not finite and > 0", (double)mp->iso);
  VoxelBox vb;
  if (int rc = check_box(c, "vx_mesh_extract", mp->box_lo, mp->box_hi, &vb)) return rc;
  const MeshBox box{{vb.lo[0], vb.lo[1], vb.lo[2]}, {vb.hi[0], vb.hi[1], vb.hi[2]}};
  if (segment && !c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_extract: source = VX_MESH_SEGMENT with no current segment (vx_segment or vx_segment_write_mask "
            "first; an upload drops it)");
  if (int rc = ensure_mesh(c)) return rc;
  c->vol.mesh_valid = false;
  c->vol.mesh_nv = c->vol.mesh_nt = 0;
  const MeshDev& m = c->vol.mesh;
  const VxParams& p = c->params;
  const float iso = segment ? 0.5f : mp->iso;
  if (int rc = c->mesh_timer.mark(c, 0)) return rc;
  if (segment) {
    const uint32_t blocks = (uint32_t)std::min<size_t>(((size_t)m.nb * 8u + 255u) / 256u, 8192u);
    hipLaunchKernelGGL(mesh_inside_segment, dim3(blocks), dim3(256), 0, c->stream, c->vol.seg.seg, box, m);
  } else {
    const uint32_t blocks = std::min<uint32_t>((m.nb + 3u) / 4u, 4096u);
    with_layout(slice_layout(c), [&](auto lay) {
      constexpr int LAY = decltype(lay)::value;
      hipLaunchKernelGGL((mesh_inside_density<LAY>), dim3(blocks), dim3(256), 0, c->stream, c->vol.dv, p.volume_density_scale,
                         p.volume_inv_maj, iso, box, m);
    });
  }
  VX_HIP(c, hipGetLastError());
  if (int rc = c->mesh_timer.mark(c, 1)) return rc;
  hipLaunchKernelGGL(mesh_active, dim3(m.np), dim3(256), 0, c->stream, m);
  hipLaunchKernelGGL(mesh_scan_partials, dim3(1), dim3(1024), 0, c->stream, m);
  hipLaunchKernelGGL(mesh_offsets, dim3(m.np), dim3(256), 0, c->stream, m);
  VX_HIP(c, hipGetLastError());
  if (int rc = c->mesh_timer.mark(c, 2)) return rc;
  MeshStats st;
  VX_HIP(c, hipMemcpyAsync(&st, m.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  const uint64_t nv = st.verts, nt = 2u * (uint64_t)st.quads;
  const uint64_t maxv = mp->max_vertices ? mp->max_vertices : 0xfffffffeull, maxt = mp->max_triangles ? mp->max_triangles : 0xfffffffeull;
  if (nv > maxv || nt > maxt)
    VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_extract: the mesh has %llu vertices and %llu triangles, more than max_vertices = %llu or "
            "max_triangles = %llu", (unsigned long long)nv, (unsigned long long)nt, (unsigned long long)maxv, (unsigned long long)maxt);
  // three values per vertex and per triangle (every earlier call has completed: each one synchronises)
  if (int rc = c->vol.mesh_verts.ensure(c, (size_t)nv * 3u)) return rc;
  if (int rc = c->vol.mesh_cells.ensure(c, (size_t)nv * 3u)) return rc;
  if (int rc = c->vol.mesh_tris.ensure(c, (size_t)nt * 3u)) return rc;
  {
    const uint32_t blocks = std::min<uint32_t>((m.ncb + 3u) / 4u, 4096u);
    if (segment)   // no voxel is read: one instance serves every layout
      hipLaunchKernelGGL((mesh_emit<LAYOUT_REF, true>), dim3(blocks), dim3(256), 0, c->stream, c->vol.dv, p.volume_density_scale, p.volume_inv_maj,
                         iso, box, m, (unsigned long long)nv, (unsigned long long)st.quads, c->vol.mesh_verts, c->vol.mesh_cells, c->vol.mesh_tris);
    else
      with_layout(slice_layout(c), [&](auto lay) {
        constexpr int LAY = decltype(lay)::value;
        hipLaunchKernelGGL((mesh_emit<LAY, false>), dim3(blocks), dim3(256), 0, c->stream, c->vol.dv, p.volume_density_scale, p.volume_inv_maj,
                           iso, box, m, (unsigned long long)nv, (unsigned long long)st.quads, c->vol.mesh_verts, c->vol.mesh_cells, c->vol.mesh_tris);
      });
  }
  VX_HIP(c, hipGetLastError());
  if (int rc = c->mesh_timer.mark(c, 3)) return rc;
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->mesh_timer.read(c)) return rc;
  c->mesh_launches = 5u;
  c->vol.mesh_nv = nv;
  c->vol.mesh_nt = nt;
  c->vol.mesh_valid = true;
  if (out) {
    VxMeshResult r{};
    r.vertices = nv;
    r.triangles = nt;
    r.active_blocks = st.active_blocks;
    r.blocks = m.ncb;
    if (nv)
      for (int a = 0; a < 3; ++a) {
        r.bbox_lo[a] = st.lo[a] - 1u;   // the statistics hold cell + 1; cell -1 wraps to its two's complement
        r.bbox_hi[a] = st.hi[a] - 1u;
      }
    *out = r;
  }
  return VX_OK;
}

int vx_mesh_read(VxContext* c, float* verts_xyz, int32_t* cells_xyz, uint32_t* tris) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_mesh_read(c->members[0], verts_xyz, cells_xyz, tris));
  VX_DEV(c);
  if (!c->vol.mesh_valid) VX_FAIL(c, VX_ERR_INVALID, "vx_mesh_read: no current mesh (vx_mesh_extract first; an upload drops it)");
  if (verts_xyz && c->vol.mesh_nv)
    VX_HIP(c, hipMemcpyAsync(verts_xyz, c->vol.mesh_verts, (size_t)c->vol.mesh_nv * 12u, hipMemcpyDeviceToHost, c->stream));
  if (cells_xyz && c->vol.mesh_nv)
    VX_HIP(c, hipMemcpyAsync(cells_xyz, c->vol.mesh_cells, (size_t)c->vol.mesh_nv * 12u, hipMemcpyDeviceToHost, c->stream));
  if (tris && c->vol.mesh_nt) VX_HIP(c, hipMemcpyAsync(tris, c->vol.mesh_tris, (size_t)c->vol.mesh_nt * 12u, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_mesh_stats(VxContext* c, uint32_t* launches, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_mesh_stats(c->members[0], launches, kernel_ms));
  if (launches) *launches = c->mesh_launches;
  if (kernel_ms) std::copy_n(c->mesh_timer.ms, 3, kernel_ms);
  return VX_OK;
}

}  // extern "C"
