// vx_slice.hpp -- slices and thick slabs (vx_slice, DESIGN.md section 2 "Slices"): one lane per output pixel, the N slab samples
// of the pixel reduced in the lane's registers.  No LDS, no atomics, no scratch.
//
// Mapping: 256-thread workgroups over 16 x 16 pixels; each wave covers one 8 x 8 block of them, so the 64 positions of one gather
// lie on a small patch of the plane and stay close together in the volume for any orientation of the plane.
#pragma once

#include "vx_modes.hpp"

namespace vx {

// A position is clamped to +-2^24 before the floor: the cell index then stays far from the int range, and every tap of a clamped
// position is outside the volume (extents are far below 2^24), as it was before the clamp -- the value is unchanged.
constexpr float SLICE_Q_MAX = 16777216.0f;

// the byte of a display component: (uint8_t)(c * 255 + 0.5) of c clamped to [0, 1]
VXD uint32_t slice_byte(float c) { return (uint32_t)(gl_clamp(c, 0.0f, 1.0f) * 255.0f + 0.5f); }

template <int REDUCE, int LAYOUT>
__global__ __launch_bounds__(256) void slice_reduce(const VxSliceParams sp, const DevVolume v, float density_scale, float inv_maj,
                                                    const float4* __restrict__ tf, uint32_t tf_len, float sr0, float sr1,
                                                    float* __restrict__ values, uchar4* __restrict__ rgba) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  const uint32_t W = sp.size[0], H = sp.size[1];
  if (x >= W || y >= H) return;
  const float fx = (float)x, fy = (float)y;
  const float bx = fma_(fy, sp.dv[0], fma_(fx, sp.du[0], sp.origin[0]));
  const float by = fma_(fy, sp.dv[1], fma_(fx, sp.du[1], sp.origin[1]));
  const float bz = fma_(fy, sp.dv[2], fma_(fx, sp.du[2], sp.origin[2]));
  auto density = [&](float fs) {
    const float qx = fminf(fmaxf(fma_(fs, sp.dn[0], bx), -SLICE_Q_MAX), SLICE_Q_MAX);
    const float qy = fminf(fmaxf(fma_(fs, sp.dn[1], by), -SLICE_Q_MAX), SLICE_Q_MAX);
    const float qz = fminf(fmaxf(fma_(fs, sp.dn[2], bz), -SLICE_Q_MAX), SLICE_Q_MAX);
    const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
    return trilinear_cell<LAYOUT>(v, density_scale, f2i(flx), f2i(fly), f2i(flz), qx - flx, qy - fly, qz - flz) * inv_maj;
  };
  const float nf = (float)sp.slab_samples;   // <= 4096: exact
  float acc = density(0.0f);
  for (float fs = 1.0f; fs < nf; fs += 1.0f) {
    const float d = density(fs);
    if (REDUCE == VX_SLICE_MEAN) acc = acc + d;
    else if (REDUCE == VX_SLICE_MAX) acc = fmaxf(acc, d);
    else acc = fminf(acc, d);
  }
  const float value = REDUCE == VX_SLICE_MEAN ? acc / nf : acc;
  const size_t o = (size_t)y * W + x;
  values[o] = value;
  if (sp.display == VX_SLICE_GREY) {   // wave uniform (a kernel argument)
    const uint32_t g = slice_byte((value - sp.window[0]) / (sp.window[1] - sp.window[0]));
    rgba[o] = make_uchar4((uint8_t)g, (uint8_t)g, (uint8_t)g, 255);
  } else if (sp.display == VX_SLICE_TF) {
    const TfView tv{tf, tf_len, (float)tf_len, false};
    const float4 c = lookup_transfer(tv, sr0, sr1, value);
    rgba[o] = make_uchar4((uint8_t)slice_byte(c.x * c.w), (uint8_t)slice_byte(c.y * c.w), (uint8_t)slice_byte(c.z * c.w), 255);
  }
}

}  // namespace vx
