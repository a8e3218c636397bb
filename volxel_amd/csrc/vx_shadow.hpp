// vx_shadow.hpp -- shadowed DVR (VxParams::dvr_shadow_stride, DESIGN.md section 2 "light grid"): the build of the light grid
// and the generic shadowed DVR kernel.  The LDS-window form of the shadowed march is render_dvr_lds_shadow (vx_dvr_lds.hpp);
// the look-up both use is shadow_lookup (vx_device.hpp).
//
// The reference's one-bounce path tracer multiplies every light sample by the transmittance toward the directional light
// (fragment.frag:92-97, environment.glsl:30-33); DVR drops that term.  All light rays are parallel, so the transmittance is a
// smooth field that one march per lattice node tabulates, and a contributing DVR sample reads it back trilinearly.
#pragma once

#include "vx_modes.hpp"
#include "vx_kernels.hpp"

namespace vx {

// the light march, the same for every node (vx_api.hip light_march): computed once on the host
struct LightMarch {
  float idir[3];     // mat3(density_transform_inv) * (-light_dir)
  float dt;          // dvr_step_voxels / |idir|
  float box_lo[3];   // the clip box (volume_aabb) in index space
  float box_hi[3];
  uint32_t stride;   // s
  uint32_t n[3];     // nodes per axis
  uint32_t ilo[3];   // per axis the first and last node whose position s * i + 1/2 lies inside the clip box (ilo <= ihi)
  uint32_t ihi[3];
};

// Block = 8 x 8 x 4 nodes, wave = a 4 x 4 x 4 block of them: the 64 parallel marches of a wave read neighbouring cells.
// Node (i, j, k): a march from index position s * (i, j, k) + 1/2 toward the light, clipped to the clip box, with the sample
// placement, densities (A5, any layout: same bits), TF alpha (A7) and optical depth of the primary DVR march; it stops at
// the first sample with tau >= dvr_ert_tau when that is > 0.  The node stores exp(-tau).  `samples` (one u64) gains the
// number of samples taken.
template <int LAYOUT>
__global__ __launch_bounds__(256) void build_light_grid(const VxParams p, const DevVolume v, const float4* __restrict__ tf_global,
                                                        uint32_t tf_len, const LightMarch lm, float* __restrict__ out,
                                                        unsigned long long* __restrict__ samples) {
  extern __shared__ float4 tf_lds[];
  TfView tf;
  tf.len = tf_len;
  tf.lenf = (float)tf_len;
  if (tf_len <= TF_LDS_MAX) {
    for (uint32_t i = threadIdx.x; i < tf_len; i += blockDim.x) tf_lds[i] = tf_global[i];
    __syncthreads();
    tf.lut = tf_lds;
    tf.in_lds = true;
  } else {
    tf.lut = tf_global;
    tf.in_lds = false;
  }
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t i = blockIdx.x * 8u + (wave & 1u) * 4u + (lane & 3u);
  const uint32_t j = blockIdx.y * 8u + (wave >> 1) * 4u + ((lane >> 2) & 3u);
  const uint32_t k = blockIdx.z * 4u + (lane >> 4);
  const bool node = i < lm.n[0] && j < lm.n[1] && k < lm.n[2];
  const float sf = (float)lm.stride;
  const V3 o = v3(fma_(sf, (float)i, 0.5f), fma_(sf, (float)j, 0.5f), fma_(sf, (float)k, 0.5f));   // exact: small integers
  const V3 idir = v3(lm.idir[0], lm.idir[1], lm.idir[2]);
  float near = 0.0f, far = 0.0f;
  const bool hit = node && ray_box_intersection(Ray{o, idir}, lm.box_lo, lm.box_hi, near, far);   // near = max(., 0)
  const float dt = lm.dt;
  const float t0 = fma_(0.5f, dt, near);
  const float x = (far - t0) / dt;
  const float nf = (hit && x > 0.0f) ? fminf(ceilf(x), (float)p.dvr_max_steps) : 0.0f;
  const V3 dq = v3(dt * idir.x, dt * idir.y, dt * idir.z);
  const V3 q0 = v3(fma_(t0, idir.x, o.x) - 0.5f, fma_(t0, idir.y, o.y) - 0.5f, fma_(t0, idir.z, o.z) - 0.5f);
  const float scale = p.volume_density_scale, inv_maj = p.volume_inv_maj, maj = p.volume_maj;
  const float sr0 = p.sample_range[0], sr1 = p.sample_range[1], ert = p.dvr_ert_tau;
  float tau = 0.0f, kf = 0.0f;
#pragma unroll 1
  for (; kf < nf; kf += 1.0f) {
    const float qx = fma_(kf, dq.x, q0.x), qy = fma_(kf, dq.y, q0.y), qz = fma_(kf, dq.z, q0.z);
    const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
    const float d = trilinear_cell<LAYOUT>(v, scale, f2i(flx), f2i(fly), f2i(flz), qx - flx, qy - fly, qz - flz);
    const float a = lookup_transfer_alpha(tf, sr0, sr1, d * inv_maj);
    tau = fma_(a * maj, dt, tau);
    if (ert > 0.0f && tau >= ert) { kf += 1.0f; break; }
  }
  if (node) out[(k * lm.n[1] + j) * lm.n[0] + i] = expf(-tau);
  const uint32_t n = wave_sum((uint32_t)kf);   // kf <= 2^24 per node, 64 nodes: exact
  if (lane == 0u && n != 0u) atomicAdd(samples, (unsigned long long)n);
}

// Shadowed DVR on the generic march (Frame::dvr<false, true>): where the LDS-window kernel does not run -- the REFERENCE and
// CELLQUAD layouts, dvr_ert_tau <= 0, a TF longer than TF_LDS_MAX.  One pixel per lane as render_generic<VX_MODE_DVR>; DVR
// launches of render_generic never fold the running mean (vx_api.hip folds), neither does this one.
template <int LAYOUT>
__global__ __launch_bounds__(256) void render_generic_shadow(const VxParams p, const DevVolume v, const float4* __restrict__ tf_global,
                                                             uint32_t tf_len, const MultiOut mo, float weight, const TileMap tm,
                                                             const ShadowGrid sg) {
  extern __shared__ float4 tf_lds[];
  TfView tf;
  tf.len = tf_len;
  tf.lenf = (float)tf_len;
  if (tf_len <= TF_LDS_MAX) {
    for (uint32_t i = threadIdx.x; i < tf_len; i += blockDim.x) tf_lds[i] = tf_global[i];
    __syncthreads();
    tf.lut = tf_lds;
    tf.in_lds = true;
  } else {
    tf.lut = tf_global;
    tf.in_lds = false;
  }
  uint32_t fslot, blk;
  multi_slot(blockIdx.x, mo.count, fslot, blk);
  float4* __restrict__ slab = mo.out[fslot];
  DevCounters* __restrict__ dc = mo.dc[fslot];
  const uint32_t frame = mo.frame[fslot];
  uint32_t lt, sub;
  if (!block_to_tile(blk, tm, lt, sub)) return;
  const uint32_t wt = sub * 4u + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
  int px, py;
  uint32_t si;
  const bool active = wave_pixel(tm, lt, wt, lane, px, py, si);
  Counts c{0, 0, 0, 0, 0};
  if (active) {
    Frame<LAYOUT> f{p, v, tf, c, sg};
    const float4 r = f.template shade_pixel<VX_MODE_DVR, true>(px, py, frame);
    float4 prev = make_float4(0.f, 0.f, 0.f, 0.f);
    if (weight != 0.0f) prev = slab[si];
    float4 o;   // fragment.frag:158, as render_generic
    o.x = fma_(1.0f - weight, r.x, weight * prev.x);
    o.y = fma_(1.0f - weight, r.y, weight * prev.y);
    o.z = fma_(1.0f - weight, r.z, weight * prev.z);
    o.w = 1.0f;
    slab[si] = o;
  }
  flush_counts(dc, c, active ? 1u : 0u, blk);
}

}  // namespace vx
