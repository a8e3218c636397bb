// vx_dvr_lds.hpp -- DVR (VX_MODE_DVR) and DVR + central-difference gradient + Blinn-Phong (VX_MODE_DVR_PHONG,
// BASELINE config 4) on the "brickf32" layout: 8^3 bricks of decoded fp32 voxels in HBM, the active window of
// voxels staged per wave through LDS ("volume laid out in 8^3 bricks, per-workgroup LDS staging of the active
// brick", BASELINE north star).
//
// Why LDS: the cellquad kernel (vx_dvr.hpp) is bound by the vector L1's tag pipe -- the 64 lanes of a gather touch
// ~10 distinct 128-byte lines but the L1 works on groups of 4 lanes and spends ~30 look-ups on them (bench.py
// roofline.l1).  Here a wave fetches every voxel of its window ONCE with row-coalesced 16-byte loads (3 load
// instructions per window of ~16 march steps instead of 2 per march step) and then takes the eight taps of a sample -- and the 24
// further taps of a gradient -- from LDS, which has no tags.
//
// One wave = one 8x8-pixel tile, as everywhere.  Per window:
//   1. anchor: the window is DIMX x DIMY x DIMZ voxels; per axis it starts at the smallest cell any live lane
//      samples next (largest, if the wave marches in the negative direction), x rounded down to a multiple of 4;
//   2. stage: lane = one (y,z) row of the window: X / 4 aligned 16-byte loads from the brick rows it crosses,
//      all issued back to back, then as many ds_write_b128; rows and chunks outside the volume are zeros (A4);
//   3. march: up to S steps; a lane takes a step while the cell of its next sample (and, for Phong, the cells one
//      voxel either side) lies inside the window, otherwise it waits for the next window.  Lanes advance at their
//      own pace -- every ray still evaluates exactly its own sample sequence, so densities, TF bins, sample counts
//      and termination are bit-identical to Frame<>::dvr and to the oracle.
// No barriers: the tile is private to the wave.
#pragma once
#include <type_traits>

#include "vx_dvr.hpp"

namespace vx {

// Window geometry (measured on config 3 / 4, 1x MI355X, 16 frames per launch, ms per frame DVR / Phong:
//   X 16, D 10 / 12, natural strides (16, 160)        0.498 / 0.838   a third of the time in LDS bank conflicts
//   X 16, D 9 / 10, strides (20, 188 / 220)            0.485 / 0.670   (+ hardware transcendentals in the shading)
//   X 16, D 8 / 10                                      0.453 / 0.664   64 rows = ONE staging pass, 6 blocks per CU
//   X 12, D 8 / 10                                      0.438 / 0.614   three chunks per row instead of four
//   X 12, D 8 / 11 (shipped)                            0.438 / 0.591
//   D 10 for DVR 0.534, S 12 / 20 / 24 / 32 steps per window 0.446 / 0.462 / 0.487 / 0.496 (S = 16: 0.438)).
// X voxels per row are staged as aligned 16-byte chunks; a row occupies RS words of LDS and a z slice SS words.
// RS = 4 (mod 8) and SS = 28 (mod 32) spread the lanes of a read over the 32 banks: eight consecutive rows land on
// eight different 4-bank groups, slices step by 28 banks.  (-DVX_LDS_X / _D / _DP / _S rebuild a variant:
// tools/variant_build.sh.)
#ifndef VX_LDS_D
#define VX_LDS_D 8
#endif
#ifndef VX_LDS_DP
#define VX_LDS_DP 10
#endif
#ifndef VX_LDS_X
#define VX_LDS_X 12
#endif
#ifndef VX_LDS_S
#define VX_LDS_S 16
#endif
#ifndef VX_LDS_S_PHONG   // steps per window of the shading kernel: with one frame's 64 pixels per wave 12 / 16 / 20 / 24 gave
#define VX_LDS_S_PHONG 16  // 0.365 / 0.370 / 0.375 / 0.377 ms per frame; with lanes = pixels x frames 12 / 16 / 20: 0.335 / 0.327 / 0.329
#endif
template <bool PHONG>
struct LdsTile {
  static constexpr int X = VX_LDS_X;             // X / 4 chunks of 16 bytes per row
#ifndef VX_LDS_DY   // windows that are not square in (y, z), with lanes = pixels x frames, config 3, ms per frame at 32 frames per
                    // launch: 8x8 0.2098, 6x10 0.2120, 10x6 0.2241, 7x9 0.2115, 9x7 0.2180; steps per window 16 / 20 / 24 / 32:
                    // 0.2110 / 0.2113 / 0.2120 / 0.2119; X = 8: 0.2255 -- the cube stays
#define VX_LDS_DY VX_LDS_D
#endif
#ifndef VX_LDS_DZ
#define VX_LDS_DZ VX_LDS_D
#endif
  static constexpr int Y = PHONG ? VX_LDS_DP : VX_LDS_DY;
  static constexpr int Z = PHONG ? VX_LDS_DP : VX_LDS_DZ;
  static constexpr int RS = (X % 8 == 4) ? X : X + 4;             // row stride in words, = 4 mod 8
  static constexpr int SS = (Y * RS + 31 - 28) / 32 * 32 + 28;    // slice stride in words: >= Y * RS, = 28 mod 32
  static constexpr int ROWS = Y * Z;
  static constexpr int FLOATS = SS * Z;          // 3968 B (DVR) / 4960 B (Phong) per wave
  static constexpr int PASSES = (ROWS + 63) / 64;
  static constexpr int LO_MARGIN = PHONG ? 1 : 0;   // cells below the sample's cell that must be resident
  static constexpr int HI_MARGIN = PHONG ? 2 : 1;   // taps above it (x+1; x+2 for the gradient)
  static_assert(SS >= Y * RS && SS % 4 == 0 && RS % 4 == 0 && RS >= X && X % 4 == 0, "tile strides");
};

// ---- wave64 integer min / max with DPP (row scan + row broadcasts), result in every lane ----
template <int CTRL, int ROW_MASK, int BANK_MASK>
VXD int dpp_src(int identity, int v) {
  return __builtin_amdgcn_update_dpp(identity, v, CTRL, ROW_MASK, BANK_MASK, false);
}
template <bool IS_MIN>
VXD int wave_minmax(int v) {
  constexpr int ID = IS_MIN ? 0x7fffffff : (int)0x80000000;
  auto op = [](int a, int b) { return IS_MIN ? (a < b ? a : b) : (a > b ? a : b); };
  v = op(v, dpp_src<0x111, 0xf, 0xf>(ID, v));  // row_shr:1
  v = op(v, dpp_src<0x112, 0xf, 0xf>(ID, v));  // row_shr:2
  v = op(v, dpp_src<0x114, 0xf, 0xf>(ID, v));  // row_shr:4
  v = op(v, dpp_src<0x118, 0xf, 0xf>(ID, v));  // row_shr:8   -> lane 15 of each row = row result
  v = op(v, dpp_src<0x142, 0xa, 0xf>(ID, v));  // row_bcast:15 into rows 1 and 3
  v = op(v, dpp_src<0x143, 0xc, 0xf>(ID, v));  // row_bcast:31 into rows 2 and 3
  return __builtin_amdgcn_readlane(v, 63);
}

// three minima at once, the stages of the three chains interleaved: a DPP instruction must wait two cycles for the
// instruction that wrote its source, and three independent chains fill those slots with work instead of s_nop
VXD void wave_min3(int& a, int& b, int& c) {
  constexpr int ID = 0x7fffffff;
  auto mn = [](int x, int y) { return x < y ? x : y; };
#define VX_STAGE(CTRL, RM)                              \
  {                                                     \
    const int ta = dpp_src<CTRL, RM, 0xf>(ID, a), tb = dpp_src<CTRL, RM, 0xf>(ID, b), tc = dpp_src<CTRL, RM, 0xf>(ID, c); \
    a = mn(a, ta); b = mn(b, tb); c = mn(c, tc);        \
  }
  VX_STAGE(0x111, 0xf) VX_STAGE(0x112, 0xf) VX_STAGE(0x114, 0xf) VX_STAGE(0x118, 0xf) VX_STAGE(0x142, 0xa) VX_STAGE(0x143, 0xc)
#undef VX_STAGE
  a = __builtin_amdgcn_readlane(a, 63);
  b = __builtin_amdgcn_readlane(b, 63);
  c = __builtin_amdgcn_readlane(c, 63);
}

// one trilinear mix of eight taps, common.glsl:62-68 (without the density scale)
VXD float mix8(float v000, float v100, float v010, float v110, float v001, float v101, float v011, float v111,
               float fx, float wx, float fy, float wy, float fz, float wz) {
  float lx0 = fma_(v100, fx, v000 * wx);
  float lx1 = fma_(v110, fx, v010 * wx);
  float hx0 = fma_(v101, fx, v001 * wx);
  float hx1 = fma_(v111, fx, v011 * wx);
  float l = fma_(lx1, fy, lx0 * wy);
  float h = fma_(hx1, fy, hx0 * wy);
  return fma_(h, fz, l * wz);
}

// occupancy asked of the register allocator: the DVR build fits 61 VGPRs without a scratch access and gains from 8 resident
// waves per SIMD (ms per frame at 5 / 6 / 7 / 8 waves: 0.434 / 0.431 / 0.420 / 0.415); the Phong build needs 86
#ifndef VX_W_LDS
#define VX_W_LDS 8
#endif
// with the 8 KB macro-cell mask beside the tiles six workgroups fit a CU: 6 waves per SIMD, 80 VGPRs
#ifndef VX_W_LDS_SKIP
#define VX_W_LDS_SKIP 6
#endif
#ifndef VX_W_LDS_PHONG
#define VX_W_LDS_PHONG 7
#endif
typedef const float __attribute__((address_space(3))) * LdsFloatPtr;

// U8: the window is staged from the bricku8 layout (8-bit codes + a range per brick, decoded here with A4's fma) instead
// of brickf32's fp32 voxels -- the dword index of a 4-voxel chunk is brickf32's 16-byte-unit index, so the row and chunk
// arithmetic is shared; everything after the staging is the same code on the same values.
template <int S, bool PHONG, bool SKIP, bool U8 = false>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PHONG ? (SKIP ? 1 : VX_W_LDS_PHONG) : (SKIP ? VX_W_LDS_SKIP : VX_W_LDS), 8))) void render_dvr_lds(const VxParams p, const DevVolume v,
                                                       const float4* __restrict__ tf_global, uint32_t tf_len,
                                                       const MultiOut mo, float weight, const TileMap tm,
                                                       const uint32_t* __restrict__ order) {
  constexpr bool SHADOW = false;
  constexpr int PROJ = 0;
  const ShadowGrid sg{};
  const float* const pbound = nullptr;
  constexpr bool SEGV = false;
  [[maybe_unused]] const uint32_t* const segm = nullptr;
  [[maybe_unused]] const uint32_t seg_inv = 0u;
#include "vx_dvr_lds_march.inc"
}
// The segment view (VX_SEGVIEW_ONLY / _HIDE, DESIGN.md section 2 "Segment views"): the same march on the masked volume -- the
// staging zeroes a voxel whose bit of the segment mask `segm` (brick-major, 8 x u64 per brick, as vx_segment.hpp) XOR `seg_inv`
// (0: ONLY, ~0u: HIDE) is 0.  No range skipping: the skip bits are built from the unmasked bricks' ranges.  A kernel of its own,
// as the shadowed form: the kernels above stay the code they were.
template <int S, bool PHONG, bool U8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(PHONG ? VX_W_LDS_PHONG : VX_W_LDS, 8))) void render_dvr_lds_seg(
    const VxParams p, const DevVolume v, const float4* __restrict__ tf_global, uint32_t tf_len, const MultiOut mo, float weight,
    const TileMap tm, const uint32_t* __restrict__ order, const uint32_t* __restrict__ segm, const uint32_t seg_inv) {
  constexpr bool SKIP = false;
  constexpr bool SHADOW = false;
  constexpr int PROJ = 0;
  const ShadowGrid sg{};
  const float* const pbound = nullptr;
  constexpr bool SEGV = true;
#include "vx_dvr_lds_march.inc"
}
// Shadowed DVR (VxParams::dvr_shadow_stride): the same march, and a contributing sample adds w = dT * T_L,
// T_L the trilinear look-up of the light grid `sg` at the sample's position -- inside the in-range block only, where the
// composite runs anyway.  A kernel of its own, not a runtime branch (the unshadowed kernels stay the code they were), and a
// name of its own (tools/isa_cost.py finds the headline kernel by the prefix of render_dvr_lds<16, false, false, false>).
template <int S, bool SKIP, bool U8>
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(SKIP ? VX_W_LDS_SKIP : VX_W_LDS, 8))) void render_dvr_lds_shadow(
    const VxParams p, const DevVolume v, const float4* __restrict__ tf_global, uint32_t tf_len, const MultiOut mo, float weight,
    const TileMap tm, const uint32_t* __restrict__ order, const ShadowGrid sg) {
  constexpr bool PHONG = false;
  constexpr bool SHADOW = true;
  constexpr int PROJ = 0;
  const float* const pbound = nullptr;
  constexpr bool SEGV = false;
  [[maybe_unused]] const uint32_t* const segm = nullptr;
  [[maybe_unused]] const uint32_t seg_inv = 0u;
#include "vx_dvr_lds_march.inc"
}

}  // namespace vx
