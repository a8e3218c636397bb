// vx_projection.hpp -- maximum- and minimum-intensity projection (VX_MODE_MIP / VX_MODE_MINIP) on the
// brickf32 / bricku8 layouts: the LDS-window march of vx_dvr_lds_march.inc with `PROJ` set.  The window is staged exactly as
// render_dvr_lds stages it and every tap comes from LDS; per sample the kernel keeps one v_max_f32 / v_min_f32 instead of the TF
// look-up and the composite, has no early ray termination, and reads the TF once per pixel after the march.  The other layouts,
// debug_hits, VX_DVR_KERNEL=generic and TFs too long for LDS go to render_generic<VX_MODE_MIP / VX_MODE_MINIP> (Frame::project).
#pragma once
#include "vx_dvr_lds.hpp"

namespace vx {

// Range skipping (SKIP): `pbound` holds ONE float per macro cell of the empty-space grid (v.skip_level / v.skip_dims), the upper
// density bound for MIP and the lower one for MinIP (vx_host.hpp compute_projection_bounds).  It stays in global memory and is
// read through the caches: 65 536 cells x 4 B does not fit beside the TF and the tiles in a CU's 160 KB of LDS, a table rounded
// to 8 or 16 bits would skip less, and the bound is only read in free flight -- once per lane and flight round before a window
// is placed, not per march step -- where one cached load per lane is small against the window it saves.
template <int S, bool MINIP, bool SKIP, bool U8>
// Occupancy asked of the register allocator: 8 waves per SIMD, as the DVR build; the SKIP builds on brickf32 came out with a
// 36-byte stack frame under that budget, so they are asked for VX_W_LDS_SKIP like the DVR SKIP builds (see the resource report
// in NOTEBOOK.md).
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SKIP ? VX_W_LDS_SKIP : VX_W_LDS, 8))) void render_proj_lds(
    const VxParams p, const DevVolume v, const float4* __restrict__ tf_global, uint32_t tf_len, const MultiOut mo, float weight,
    const TileMap tm, const uint32_t* __restrict__ order, const float* __restrict__ pbound) {
  constexpr bool PHONG = false;
  constexpr bool SHADOW = false;
  constexpr int PROJ = MINIP ? 2 : 1;
  const ShadowGrid sg{};
  constexpr bool SEGV = false;
  [[maybe_unused]] const uint32_t* const segm = nullptr;
  [[maybe_unused]] const uint32_t seg_inv = 0u;
#include "vx_dvr_lds_march.inc"
}
// the segment view (render_dvr_lds_seg, vx_dvr_lds.hpp): the projection of the masked volume, without range skipping (the bound
// table is built from the unmasked bricks).  MinIP sees the hidden voxels' zeros.
template <int S, bool MINIP, bool U8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(VX_W_LDS, 8))) void render_proj_lds_seg(
    const VxParams p, const DevVolume v, const float4* __restrict__ tf_global, uint32_t tf_len, const MultiOut mo, float weight,
    const TileMap tm, const uint32_t* __restrict__ order, const uint32_t* __restrict__ segm, const uint32_t seg_inv) {
  constexpr bool SKIP = false;
  constexpr bool PHONG = false;
  constexpr bool SHADOW = false;
  constexpr int PROJ = MINIP ? 2 : 1;
  const ShadowGrid sg{};
  const float* const pbound = nullptr;
  constexpr bool SEGV = true;
#include "vx_dvr_lds_march.inc"
}

}  // namespace vx
