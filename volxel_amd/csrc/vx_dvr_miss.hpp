// vx_dvr_miss.hpp -- the light half of a split DVR launch: the blocks of 16x16 pixels the host proved no primary ray can hit
// the clip box from (vx_host.hpp classify_miss_blocks).  A pixel whose ray misses the box has C = 0 and
// T = 1: its radiance is the environment term alone, so it needs its jitter, its world-space direction and the fold -- not the
// index transform, the step bound, dt, the reciprocals, a window, the wave's tile or the transfer function in LDS.
// A kernel of its own, as the shadowed form and the segment view: the kernels of vx_dvr_lds.hpp stay the code they were.
// No slab test here: that no lane hits is the host's proof, and nothing below depends on it being re-checked.
#pragma once
#include "vx_dvr_lds.hpp"

namespace vx {

// the world-space direction of dvr_setup's ray: its tex_coord, its draws in their order (the two draws behind them -- the
// tau_target slot and the start jitter -- move nothing a missing ray uses), its setup_world_ray
VXD V3 dvr_miss_dir(const VxParams& p, const DevVolume& v, int px, int py, uint32_t frame) {
  float tex_x = tex_coord(px, p.res[0], &v, 0);
  float tex_y = tex_coord(py, p.res[1], &v, 1);
  float jx = 0.5f, jy = 0.5f;
  if (p.dvr_jitter) {
    Rng s = seed_xoshiro(tea32(42u * (uint32_t)(py * p.res[0] + px), frame));
    float a0 = rng(s), a1 = rng(s), b0 = rng(s), b1 = rng(s);
    jx = (a0 + b0) / 2.0f;
    jy = (a1 + b1) / 2.0f;
  }
  return setup_world_ray(p, tex_x, tex_y, jx, jy, &v).d;
}

// The argument list of render_dvr_lds (lane_frame_slot and fold_frames read the frame slots and the weights from the
// kernel-argument segment at its offsets); tf_global and tf_len are not used.  `order` lists the launch's blocks.  The wave's
// pixels x frames are the LDS-window kernel's: multi_slot, frame_group<6> when the launch folds and <VX_DVR_FL_MAXSH>
// otherwise, wave_pixel.  Multi-frame launches only (plan_launch).  64 VGPRs at most (8 waves per SIMD), no scratch; dynamic
// LDS: 5 KiB per workgroup for the fold in a launch that folds, none otherwise.
__global__ __launch_bounds__(256) __attribute__((amdgpu_waves_per_eu(8, 8))) void render_dvr_miss(
    const VxParams p, const DevVolume v, const float4* __restrict__ tf_global, uint32_t tf_len, const MultiOut mo, float weight,
    const TileMap tm, const uint32_t* __restrict__ order) {
  extern __shared__ float fold_lds[];   // fold_frames' scratch, 320 floats per wave (mo.fuse != 0 only)
  uint32_t fslot, bslot;
  multi_slot(blockIdx.x, mo.count, fslot, bslot);
  const uint32_t blk = order[bslot];
  float4* __restrict__ slab = mo.out[fslot];
  DevCounters* __restrict__ dc = mo.dc[fslot];
  uint32_t lt, sub;
  if (!block_to_tile(blk, tm, lt, sub)) return;
  const uint32_t wt = sub * 4u + (threadIdx.x >> 6);
  const uint32_t lane = threadIdx.x & 63u;
  uint32_t plane = lane, my_frame = mo.frame[fslot];
  const uint32_t fuse = mo.fuse;
  if (mo.count > 1u) {   // lanes = pixels x frames, as vx_dvr_lds_march.inc
    uint32_t base;
    const uint32_t sh = fuse ? frame_group<6>(fslot, mo.count, base) : frame_group<VX_DVR_FL_MAXSH>(fslot, mo.count, base);
    if (sh != 0u) {
      const uint32_t psh = 6u - sh;
      plane = ((fslot - base) << psh) + (lane & ((1u << psh) - 1u));
      slab = lane_frame_slot(base + (lane >> psh), my_frame);
    }
  }
  int px, py;
  uint32_t si;
  const bool in_image = wave_pixel(tm, lt, wt, plane, px, py, si);
  DvrRay r{};
  if (in_image) r.wdir = dvr_miss_dir(p, v, px, py, my_frame);
  if (fuse != 0u) {
    V3 L = v3(0.f, 0.f, 0.f);
    if (in_image) L = dvr_radiance(p, v, r, 0.0f, 0.0f, 0.0f, 1.0f);
    fold_frames(fold_lds + (threadIdx.x >> 6) * 320u, lane, L, in_image, si, mo.accum, fuse, 31u - (uint32_t)__builtin_clz(mo.count));
  } else if (in_image) dvr_store(p, v, r, 0.0f, 0.0f, 0.0f, 1.0f, weight, slab, si);
  const uint32_t n_px = (uint32_t)__builtin_popcountll(ballot(in_image));
  add_counts(dc, 0u, 0u, n_px, 0u, 0u, 0u, blk);
}

// The block order of a split launch: a stable partition of `order` (a permutation of the n logical blocks, longest first) into
// the blocks that may hit (miss[b] == 0) and the rest, so that the LDS-window kernel still starts its longest blocks first.
// One workgroup; n is a frame's block count (8192 at 1920x1080).
__global__ __launch_bounds__(1024) void split_order(const uint32_t* __restrict__ order, const uint8_t* __restrict__ miss, uint32_t n,
                                                     uint32_t* __restrict__ heavy, uint32_t* __restrict__ light) {
  __shared__ uint32_t cnt[1024];
  const uint32_t per = (n + 1023u) / 1024u;
  const uint32_t lo = min(threadIdx.x * per, n), hi = min(lo + per, n);
  auto is_miss = [&](uint32_t b) { return b < n && miss[b] != 0; };
  uint32_t m = 0;
  for (uint32_t i = lo; i < hi; ++i) m += is_miss(order[i]) ? 1u : 0u;
  cnt[threadIdx.x] = m;
  __syncthreads();
  for (uint32_t off = 1; off < 1024u; off <<= 1) {   // inclusive scan
    const uint32_t add = threadIdx.x >= off ? cnt[threadIdx.x - off] : 0u;
    __syncthreads();
    cnt[threadIdx.x] += add;
    __syncthreads();
  }
  uint32_t mpos = cnt[threadIdx.x] - m, hpos = lo - mpos;   // misses / hits before this thread's run: both below n
  for (uint32_t i = lo; i < hi; ++i) {
    const uint32_t b = order[i];
    if (is_miss(b)) light[mpos++] = b;
    else heavy[hpos++] = b;
  }
}

}  // namespace vx
