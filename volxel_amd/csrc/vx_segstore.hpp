// vx_segstore.hpp -- the kernels of the segment store (vx_segment_combine, vx_segment_compare, vx_segments_labelmap; DESIGN.md
// section 2 "Segment store"): what needs two or more brick-major bit masks of vx_segment.hpp present at once.  A is the current
// segment (SegDev::seg), B the words of a slot; every mask is nb * 8 words, an even number.
//
//   sst_combine      A = op(A, B), word-wise and in place, two words per lane and step: each lane reads the words it writes and
//                    no other, so in place is exact.  INVERT reads no B.
//   sst_count / sst_count_final   |A|, |B| and |A & B|: popcounts summed per lane, per wave by 64-lane shuffles, per workgroup
//                    over LDS into one partial; one workgroup adds the partials.  Integer sums: exact in any order.
//   sst_max_over     behind an uncapped transform of one set (vx_distance.hpp): the largest D2 of the field over the voxels of
//                    the OTHER set and the C-order-first voxel that attains it, +inf included (the transform of an empty set),
//                    into the partials dst_reduce_final merges.  Ties break as dst_reduce breaks them (dst_merge).  A word
//                    without a voxel of the set reads nothing of the field.
//   sst_labelmap     the dense (Z, Y, X) uint8 label map of up to VX_SEGMENT_SLOTS masks in list order: one lane per 8-voxel row
//                    of a brick writes its 8 labels as one 8-byte store; the voxels held by more than one mask are counted per
//                    lane, summed per wave by shuffles and added once per wave to one counter the host zeroed.
// The discipline of vx_segment.hpp holds: plain vector loads and stores, one writer per destination per launch, no spin, no
// grid barrier, no cooperative or persistent launch.
#pragma once

#include "vx_distance.hpp"

namespace vx {

// the sum of v over the 64 lanes of a wave, in lane 0
VXD unsigned long long sst_wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d, 64);
  return v;
}

VXD uint64_t sst_op(int op, uint64_t a, uint64_t b) {
  switch (op) {
    case VX_COMBINE_UNION: return a | b;
    case VX_COMBINE_INTERSECT: return a & b;
    case VX_COMBINE_SUBTRACT: return a & ~b;
    case VX_COMBINE_XOR: return a ^ b;
    default: return ~a;
  }
}

// a = op(a, b) over `pairs` pairs of words; b is not read (and may be null) for VX_COMBINE_INVERT
__global__ __launch_bounds__(256) void sst_combine(uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const int op,
                                                   const size_t pairs) {
  ulonglong2* pa = reinterpret_cast<ulonglong2*>(a);
  const ulonglong2* pb = reinterpret_cast<const ulonglong2*>(b);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < pairs; k += stride) {
    const ulonglong2 x = pa[k];
    const ulonglong2 y = op == VX_COMBINE_INVERT ? make_ulonglong2(0ull, 0ull) : pb[k];
    pa[k] = make_ulonglong2(sst_op(op, x.x, y.x), sst_op(op, x.y, y.y));
  }
}

// the sums of a workgroup's lanes: shuffles inside each of its 4 waves, then lane 0 adds the 4 wave sums from LDS
VXD SstCount sst_block_sum(SstCount p, SstCount* sh) {
  p.a = sst_wave_sum(p.a);
  p.b = sst_wave_sum(p.b);
  p.ab = sst_wave_sum(p.ab);
  if ((threadIdx.x & 63u) == 0u) sh[threadIdx.x >> 6] = p;
  __syncthreads();
  SstCount s{0ull, 0ull, 0ull};
  if (threadIdx.x == 0u)
    for (uint32_t w = 0; w < blockDim.x >> 6; ++w) {
      s.a += sh[w].a;
      s.b += sh[w].b;
      s.ab += sh[w].ab;
    }
  return s;
}

// one partial per workgroup over `pairs` pairs of words of a and b
__global__ __launch_bounds__(256) void sst_count(const uint64_t* __restrict__ a, const uint64_t* __restrict__ b, const size_t pairs,
                                                 SstCount* __restrict__ partials) {
  __shared__ SstCount sh[4];
  const ulonglong2* pa = reinterpret_cast<const ulonglong2*>(a);
  const ulonglong2* pb = reinterpret_cast<const ulonglong2*>(b);
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  SstCount p{0ull, 0ull, 0ull};
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < pairs; k += stride) {
    const ulonglong2 x = pa[k], y = pb[k];
    p.a += (unsigned)(__popcll(x.x) + __popcll(x.y));
    p.b += (unsigned)(__popcll(y.x) + __popcll(y.y));
    p.ab += (unsigned)(__popcll(x.x & y.x) + __popcll(x.y & y.y));
  }
  p = sst_block_sum(p, sh);
  if (threadIdx.x == 0u) partials[blockIdx.x] = p;
}

// one workgroup: the partials of sst_count into partials[0]
__global__ __launch_bounds__(256) void sst_count_final(SstCount* __restrict__ partials, const uint32_t count) {
  __shared__ SstCount sh[4];
  SstCount p{0ull, 0ull, 0ull};
  for (uint32_t k = threadIdx.x; k < count; k += 256u) {
    p.a += partials[k].a;
    p.b += partials[k].b;
    p.ab += partials[k].ab;
  }
  p = sst_block_sum(p, sh);   // (every lane has read its partials before lane 0 writes the first: the barrier is inside)
  if (threadIdx.x == 0u) partials[0] = p;
}

// one lane per word of `over`: the field values of its voxels into a partial (the largest value, +inf included, and the smallest
// C-order index among equal ones; DstPartial::finite is not used); one partial per workgroup, merged by dst_reduce_final
__global__ __launch_bounds__(256) void sst_max_over(const float* __restrict__ field, const uint64_t* __restrict__ over,
                                                    const uint32_t bc0, const uint32_t bc1, const uint32_t bc2,
                                                    DstPartial* __restrict__ partials) {
  __shared__ DstPartial sh[256];
  const size_t n = (size_t)bc0 * bc1 * bc2 * 8u, stride = (size_t)gridDim.x * blockDim.x;
  const size_t X = (size_t)bc0 * 8u, Y = (size_t)bc1 * 8u;
  DstPartial p{0ull, DST_NONE, 0.0f, 0u};
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint64_t w = over[k];
    if (w == 0ull) continue;
    const uint32_t b = (uint32_t)(k >> 3), z = (uint32_t)(k & 7u);
    const uint32_t bx = b % bc0, t = b / bc0, by = t % bc1, bz = t / bc1;
    const size_t row0 = (((size_t)bz * 8u + z) * Y + (size_t)by * 8u) * X + (size_t)bx * 8u;
    for (uint32_t y = 0; y < 8u; ++y) {
      const uint32_t m = (uint32_t)(w >> (y * 8u)) & 0xffu;
      if (m == 0u) continue;
      const float4* q = reinterpret_cast<const float4*>(field + row0 + (size_t)y * X);
      const float4 a = q[0], c = q[1];
      const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (uint32_t x = 0; x < 8u; ++x)
        if ((m >> x) & 1u) dst_merge(p, DstPartial{0ull, (unsigned long long)(row0 + (size_t)y * X + x), v[x], 0u});
    }
  }
  p = dst_block_merge(p, sh);
  if (threadIdx.x == 0u) partials[blockIdx.x] = p;
}

// the 8 bits of m as 8 bytes of 0 / 1, bit x in byte x: the product puts m in every byte, the mask keeps bit x of byte x, and
// adding 0x7f carries any kept bit into bit 7 of its own byte (0x80 + 0x7f = 0xff: never beyond it)
VXD uint64_t sst_spread(uint32_t m) {
  const uint64_t one = ((uint64_t)m * 0x0101010101010101ull) & 0x8040201008040201ull;
  return ((one + 0x7f7f7f7f7f7f7f7full) >> 7) & 0x0101010101010101ull;
}

// thread t = (row, bx), bx fastest, row = z * Y + y: the labels of voxels x = 8 bx .. 8 bx + 7 of that row, 8 bytes at
// labels + row * X + 8 bx (X = 8 bc0: 8-byte aligned).  *overlaps += the voxels more than one listed mask holds.
__global__ __launch_bounds__(256) void sst_labelmap(const SstSlots s, const uint32_t bc0, const uint32_t bc1, const uint32_t bc2,
                                                    uint8_t* __restrict__ labels, unsigned long long* __restrict__ overlaps) {
  const uint32_t Y = bc1 * 8u, rows = Y * bc2 * 8u;
  const size_t total = (size_t)rows * bc0, stride = (size_t)gridDim.x * blockDim.x;
  unsigned long long multi_n = 0;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint32_t bx = (uint32_t)(t % bc0), row = (uint32_t)(t / bc0);
    const uint32_t y = row % Y, z = row / Y;
    const size_t word = (size_t)(((z >> 3) * bc1 + (y >> 3)) * bc0 + bx) * 8u + (z & 7u);
    uint32_t seen = 0, multi = 0;
    uint64_t out = 0;
    for (uint32_t k = 0; k < s.n; ++k) {
      const uint32_t m = (uint32_t)(s.w[k][word] >> ((y & 7u) * 8u)) & 0xffu;
      out |= sst_spread(m & ~seen) * (uint64_t)(k + 1u);
      multi |= seen & m;
      seen |= m;
    }
    multi_n += (unsigned)__popc(multi);
    *reinterpret_cast<uint64_t*>(labels + t * 8u) = out;
  }
  multi_n = sst_wave_sum(multi_n);
  if ((threadIdx.x & 63u) == 0u && multi_n != 0ull) atomicAdd(overlaps, multi_n);
}

}  // namespace vx
