// vx_layout.hpp -- the kernels that build the native device layouts from the uploaded reference arrays (indirection, range,
// atlas): cellquad, brickf32, bricku8 and its per-brick ranges.  One thread per stored element over a range [first, end), so
// that an upload can build whole z layers behind the atlas chunks they read (vx_api_volume.hip, the only unit that includes
// this header).
#pragma once

#include "vx_device.hpp"

namespace vx {

// ---- reference layout -> cellquad (runs once per upload) -------------------------------
// one thread per stored quad: brick' b, slice lz in [0,9), cell (ly,lx).
// [first, end) = the quads of a range of apron-brick z layers (the upload builds the layers of an atlas chunk
// while the next chunk is still crossing PCIe)
__global__ __launch_bounds__(256) void build_cellquad(const DevVolume v, float4* __restrict__ out,
                                                       uint64_t first, uint64_t end) {
  uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= end) return;
  uint32_t q = (uint32_t)(i % CQ_BRICK_QUADS);
  uint64_t b = i / CQ_BRICK_QUADS;
  uint32_t bx = (uint32_t)(b % v.cq_bc[0]);
  uint32_t by = (uint32_t)((b / v.cq_bc[0]) % v.cq_bc[1]);
  uint32_t bz = (uint32_t)(b / ((uint64_t)v.cq_bc[0] * v.cq_bc[1]));
  // inverse of cq_cell
  uint32_t lz = q >> 6, ly = (((q >> 4) & 3u) << 1) | (q & 1u), lx = (q >> 1) & 7u;
  // voxel of local (l) in apron brick b: 8b - 1 + l
  int x = (int)(bx * 8u + lx) - 1, y = (int)(by * 8u + ly) - 1, z = (int)(bz * 8u + lz) - 1;
  float4 o;
  o.x = lookup_density_brick(v, x, y, z);
  o.y = lookup_density_brick(v, x + 1, y, z);
  o.z = lookup_density_brick(v, x, y + 1, z);
  o.w = lookup_density_brick(v, x + 1, y + 1, z);
  out[i] = o;
}

// reference layout -> brickf32: one thread per voxel of the padded grid
__global__ __launch_bounds__(256) void build_brickf32(const DevVolume v, float* __restrict__ out,
                                                       uint64_t first, uint64_t end) {
  uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= end) return;
  uint32_t l = (uint32_t)(i & 511u);
  uint64_t b = i >> 9;
  uint32_t bx = (uint32_t)(b % v.bc[0]);
  uint32_t by = (uint32_t)((b / v.bc[0]) % v.bc[1]);
  uint32_t bz = (uint32_t)(b / ((uint64_t)v.bc[0] * v.bc[1]));
  out[i] = lookup_density_brick(v, (int)(bx * 8u + (l & 7u)), (int)(by * 8u + ((l >> 3) & 7u)),
                                (int)(bz * 8u + (l >> 6)));
}

// reference layout -> bricku8: one thread per dword (4 voxels along x) of the padded grid, and one per brick range
__global__ __launch_bounds__(256) void build_bricku8(const DevVolume v, uint32_t* __restrict__ out, uint64_t first,
                                                      uint64_t end) {
  uint64_t i = first + (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;   // dword index
  if (i >= end) return;
  uint32_t l = (uint32_t)(i & 127u);        // z * 16 + y * 2 + (x >> 2)
  uint64_t b = i >> 7;
  uint32_t bx = (uint32_t)(b % v.bc[0]);
  uint32_t by = (uint32_t)((b / v.bc[0]) % v.bc[1]);
  uint32_t bz = (uint32_t)(b / ((uint64_t)v.bc[0] * v.bc[1]));
  const uint32_t x0 = bx * 8u + (l & 1u) * 4u, y = by * 8u + ((l >> 1) & 7u), z = bz * 8u + (l >> 4);
  uint32_t w = 0u;
#pragma unroll
  for (uint32_t j = 0; j < 4u; ++j) w |= lookup_code_brick(v, x0 + j, y, z) << (8u * j);
  out[i] = w;
}
__global__ __launch_bounds__(256) void build_bricku8_range(const DevVolume v, float2* __restrict__ out, uint32_t first,
                                                            uint32_t end) {
  uint32_t b = first + blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= end) return;
  const uint32_t rg = v.range[b];
  const float mn = half_bits_to_float(rg >> 16), mx = half_bits_to_float(rg & 0xffffu);
  out[b] = make_float2(mn, mx - mn);   // lookup_density_brick: fma(un, mx - mn, mn)
}

}  // namespace vx
