// vx_iso.hpp -- first-hit isosurfaces (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): one lane per pixel of the window, DVR's
// ray and march contract, the march in the lane's registers up to the first sample at or above the threshold, `refine` bisection
// steps on the sample parameter, then one Phong gradient and the Blinn-Phong colour.  No LDS windows, no scratch; the five counts
// are flushed with one atomic per wave each.
//
// Mapping: 256-thread workgroups over 16 x 16 pixels of the window; each wave covers one 8 x 8 block (as slice_reduce).  A lane
// leaves the march at its first hit; the wave runs until its longest ray is done.
#pragma once

#include "vx_modes.hpp"

namespace vx {

// The segment view (DESIGN.md section 2 "Segment views"): the decoded voxel (x, y, z) of the masked volume -- +0 where its bit of
// the brick-major segment mask (8 x u64 per brick, word z, bit y * 8 + x; read as 16 dwords, dword z * 2 + y / 4, bit
// (y & 3) * 8 + x) XOR `inv` (0: ONLY, ~0u: HIDE) is 0.  A voxel outside the volume reads 0 anyway; its mask index is clamped.
template <int LAYOUT>
VXD float seg_voxel(const DevVolume& v, const uint32_t* __restrict__ segm, uint32_t inv, int x, int y, int z) {
  const float d = lookup_density_nearest<LAYOUT>(v, x, y, z);
  const bool in = (uint32_t)x < v.extent[0] && (uint32_t)y < v.extent[1] && (uint32_t)z < v.extent[2];
  const uint32_t ux = in ? (uint32_t)x : 0u, uy = in ? (uint32_t)y : 0u, uz = in ? (uint32_t)z : 0u;
  const uint32_t b = ((uz >> 3) * v.bc[1] + (uy >> 3)) * v.bc[0] + (ux >> 3);
  const uint32_t w = segm[(size_t)b * 16u + ((uz & 7u) << 1) + ((uy & 7u) >> 2)];
  return ((w >> (((uy & 3u) << 3) | (ux & 7u))) ^ inv) & 1u ? d : 0.0f;
}
// the eight taps of cell (ix, iy, iz), mixed as trilinear_cell mixes them; SEGV: each tap through seg_voxel
template <int LAYOUT, bool SEGV>
VXD float iso_cell(const DevVolume& v, const uint32_t* __restrict__ segm, uint32_t inv, float density_scale, int ix, int iy, int iz,
                   float fx, float fy, float fz) {
  if (!SEGV) return trilinear_cell<LAYOUT>(v, density_scale, ix, iy, iz, fx, fy, fz);
  const float v000 = seg_voxel<LAYOUT>(v, segm, inv, ix, iy, iz), v100 = seg_voxel<LAYOUT>(v, segm, inv, ix + 1, iy, iz);
  const float v010 = seg_voxel<LAYOUT>(v, segm, inv, ix, iy + 1, iz), v110 = seg_voxel<LAYOUT>(v, segm, inv, ix + 1, iy + 1, iz);
  const float v001 = seg_voxel<LAYOUT>(v, segm, inv, ix, iy, iz + 1), v101 = seg_voxel<LAYOUT>(v, segm, inv, ix + 1, iy, iz + 1);
  const float v011 = seg_voxel<LAYOUT>(v, segm, inv, ix, iy + 1, iz + 1);
  const float v111 = seg_voxel<LAYOUT>(v, segm, inv, ix + 1, iy + 1, iz + 1);
  const float lx0 = gl_mix(v000, v100, fx), lx1 = gl_mix(v010, v110, fx);
  const float hx0 = gl_mix(v001, v101, fx), hx1 = gl_mix(v011, v111, fx);
  return density_scale * gl_mix(gl_mix(lx0, lx1, fy), gl_mix(hx0, hx1, fy), fz);
}

template <int LAYOUT, bool SKIP>
__global__ __launch_bounds__(256) void iso_first_hit(const VxParams p, const DevVolume v, const VxIsoParams ip, const IsoBound ib,
                                                     float4* __restrict__ rgba_out, float4* __restrict__ hit_out,
                                                     unsigned long long* __restrict__ counts) {
  constexpr bool SEGV = false;
  [[maybe_unused]] const uint32_t* const segm = nullptr;
  [[maybe_unused]] const uint32_t seg_inv = 0u;
#include "vx_iso_march.inc"
}
// the segment view: the first hit on the masked volume (iso_cell<LAYOUT, true>), without range skipping -- the bound table is
// built from the unmasked bricks' ranges; ISO_SKIPPED stays 0
template <int LAYOUT>
__global__ __launch_bounds__(256) void iso_first_hit_seg(const VxParams p, const DevVolume v, const VxIsoParams ip,
                                                         float4* __restrict__ rgba_out, float4* __restrict__ hit_out,
                                                         unsigned long long* __restrict__ counts, const uint32_t* __restrict__ segm,
                                                         const uint32_t seg_inv) {
  constexpr bool SKIP = false;
  constexpr bool SEGV = true;
  const IsoBound ib{};
#include "vx_iso_march.inc"
}

}  // namespace vx
