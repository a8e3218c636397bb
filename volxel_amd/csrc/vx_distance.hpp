// vx_distance.hpp -- the squared Euclidean distance transform of the current segment under an anisotropic spacing, and the
// millimetre margins built on it (vx_segment_distance, vx_segment_margin; DESIGN.md section 2 "Distances and margins").
//
// The field is one fp32 per voxel of index_extent, dense (z, y, x) in C order, and holds D2 -- never a square root.  The term
// of an offset of n voxels along an axis of spacing s is dst_term(n, s) = fl32(p * p), p = fl32(fl32(n) * s); a voxel's
// D2 = min over the source voxels of fl32(fl32(t_x + t_y) + t_z).  fp32 rounding is monotone, so the minimum separates
// exactly into three passes, each a plain minimum over the candidates of a line -- no lower envelope, no division:
//   dst_xpass     one lane per 8-voxel row of a brick, straight from the brick bit masks (the words sed_load8 reads, `inv`
//                 complementing them for the INSIDE side): the nearest set bit of the x row by bit operations, walking to the
//                 neighbouring bricks of the row only while the nearest bit they could hold is still within the cap's window
//                 and the volume has not ended.
//   dst_linepass  the y and the z pass, in place: a workgroup stages the whole lines of TX neighbouring x columns in LDS
//                 (row j of the tile = TX consecutive floats, so loads and stores are row-coalesced and every LDS read of a
//                 wave is one contiguous span: conflict free), then every output scans outwards from its own position,
//                 n = 1, 2, ..., taking both candidates at distance n from LDS, and stops once the term of n alone reaches the
//                 best value so far (fl32(g + t) >= t), n passes the cap's window, or the line has ended on both sides.
//                 Every line is read and written by one workgroup only, and all of a tile is staged before any of it is
//                 written, so the pass runs in place.  A value above the cap is stored as +inf: its sums only grow.
//   dst_pack      compare and pack: the brick words of { D2 <= R2 } (GROW; with `band` M | (that & P)) or of its complement
//                 (SHRINK: the field then holds the distance to the complement, which is 0 outside M).
//   dst_reduce / dst_reduce_final   the statistics of a field: the voxels with D2 <= R2, the largest finite D2 over voxels
//                 outside the source set and the C-order-first voxel that attains it.  max, and min of the index among equal
//                 maxima, are exact and associative: the two-level tree gives the same answer in any order.
// The discipline of vx_segment.hpp holds: plain vector loads and stores, one writer per destination per launch, no spin, no
// grid barrier, no cooperative or persistent launch.
#pragma once

#include "vx_segedit.hpp"

namespace vx {

constexpr float DST_INF = __builtin_huge_valf();
constexpr uint32_t DST_FAR = 0x7fffffffu;    // "no set bit on this side"
constexpr int DST_NOUT = 4;                  // outputs a lane scans together in dst_linepass (independent LDS reads in flight)

// the term of an offset of n voxels: two roundings, no contraction (-ffp-contract=off; the host evaluates the same two products)
VXD float dst_term(uint32_t n, float s) {
  const float p = (float)n * s;
  return p * p;
}

// byte (row y of word z) of brick b, complemented by inv
VXD uint32_t dst_row(const uint64_t* __restrict__ mask, uint32_t b, uint32_t z, uint32_t y, uint64_t inv) {
  return (uint32_t)(((mask[(size_t)b * 8u + z] ^ inv) >> (y * 8u)) & 0xffull);
}

// x pass: thread t = (row, bx), bx fastest: neighbouring lanes write neighbouring 32-byte pieces of one field row.
// wx = the cap's window in voxels (the largest n with dst_term(n, sx) <= R2, at most X - 1).
__global__ __launch_bounds__(256) void dst_xpass(const uint64_t* __restrict__ mask, const uint64_t inv, float* __restrict__ field,
                                                 const uint32_t bc0, const uint32_t bc1, const uint32_t bc2, const float sx,
                                                 const uint32_t wx) {
  const uint32_t Y = bc1 * 8u, rows = Y * bc2 * 8u;
  const size_t total = (size_t)rows * bc0, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x; t < total; t += stride) {
    const uint32_t bx = (uint32_t)(t % bc0), row = (uint32_t)(t / bc0);
    const uint32_t y = row % Y, z = row / Y;
    const uint32_t b = ((z >> 3) * bc1 + (y >> 3)) * bc0 + bx;
    const uint32_t m = dst_row(mask, b, z & 7u, y & 7u, inv);
    // the distance from x = 0 of this brick to the nearest set bit on its left, from x = 7 to the nearest on its right.  With a
    // bit of its own in the row no voxel is further than 7 from it, so only the facing neighbour can hold a nearer one.
    const uint32_t reach = m ? 1u : 0xffffffffu;
    uint32_t left0 = DST_FAR, right7 = DST_FAR;
    for (uint32_t k = 1; k <= bx && k <= reach && 8u * (k - 1u) + 1u <= wx; ++k) {
      const uint32_t q = dst_row(mask, b - k, z & 7u, y & 7u, inv);
      if (q) {
        left0 = 8u * (k - 1u) + (uint32_t)__clz((int)q) - 23u;   // 8 - msb(q), msb = 31 - clz
        break;
      }
    }
    for (uint32_t k = 1; bx + k < bc0 && k <= reach && 8u * (k - 1u) + 1u <= wx; ++k) {
      const uint32_t q = dst_row(mask, b + k, z & 7u, y & 7u, inv);
      if (q) {
        right7 = 8u * (k - 1u) + (uint32_t)__ffs((int)q);        // lsb(q) + 1
        break;
      }
    }
    float o[8];
#pragma unroll
    for (uint32_t x = 0; x < 8u; ++x) {
      const uint32_t below = m & ((2u << x) - 1u), above = m >> x;
      const uint32_t dl = below ? x - (31u - (uint32_t)__clz((int)below)) : (left0 == DST_FAR ? DST_FAR : x + left0);
      const uint32_t dr = above ? (uint32_t)__ffs((int)above) - 1u : (right7 == DST_FAR ? DST_FAR : 7u - x + right7);
      const uint32_t n = dl < dr ? dl : dr;
      o[x] = n <= wx ? dst_term(n, sx) : DST_INF;
    }
    float4* out = reinterpret_cast<float4*>(field + ((size_t)row * bc0 + bx) * 8u);
    out[0] = make_float4(o[0], o[1], o[2], o[3]);
    out[1] = make_float4(o[4], o[5], o[6], o[7]);
  }
}

// y / z pass.  The field is (nouter, L, X) with the line index j at stride `lstride` floats and the outer index at `ostride`
// (y pass: L = Y, lstride = X, outer = z at X * Y; z pass: L = Z, lstride = X * Y, outer = y at X).  A workgroup owns the tile
// (outer, x0 .. x0 + TX - 1): lds[j * TX + tx].  TX * JG = 256: lane (tx, jg) stages and computes the positions j = jg + JG * i.
// w = the cap's window in voxels on this axis (at most L - 1), r2 the cap itself.
template <int TX>
__global__ __launch_bounds__(256) void dst_linepass(float* __restrict__ field, const uint32_t X, const uint32_t L,
                                                    const size_t lstride, const size_t ostride, const uint32_t ntx, const float s,
                                                    const uint32_t w, const float r2) {
  extern __shared__ float lds[];
  constexpr uint32_t JG = 256u / TX;
  const uint32_t tx = threadIdx.x % TX, jg = threadIdx.x / TX;
  const uint32_t x = (blockIdx.x % ntx) * TX + tx;
  const bool live = x < X;   // (X is 8 x the brick grid; the builder's grids are multiples of 64, an uploaded brick grid need not be)
  float* col = field + (size_t)(blockIdx.x / ntx) * ostride + (live ? x : 0u);
  for (uint32_t j = jg; j < L; j += JG) lds[j * TX + tx] = live ? col[(size_t)j * lstride] : DST_INF;
  __syncthreads();
  for (uint32_t j0 = jg; j0 < L; j0 += JG * DST_NOUT) {
    float best[DST_NOUT];
    uint32_t far[DST_NOUT];     // the furthest candidate of output u: the longer side of its line, inside the window
#pragma unroll
    for (int u = 0; u < DST_NOUT; ++u) {
      const uint32_t j = j0 + u * JG;
      best[u] = j < L ? lds[j * TX + tx] : 0.0f;   // (0: an output past the end of the line asks for no candidate)
      const uint32_t side = j < L ? (j > L - 1u - j ? j : L - 1u - j) : 0u;
      far[u] = side < w ? side : w;
    }
    for (uint32_t n = 1;; ++n) {
      const float t = dst_term(n, s);
      bool go = false;
#pragma unroll
      for (int u = 0; u < DST_NOUT; ++u) {
        const uint32_t j = j0 + u * JG;
        if (n <= far[u] && t < best[u]) {
          go = true;
          if (n <= j) best[u] = fminf(best[u], lds[(j - n) * TX + tx] + t);
          if (j + n < L) best[u] = fminf(best[u], lds[(j + n) * TX + tx] + t);
        }
      }
      if (!go) break;
    }
#pragma unroll
    for (int u = 0; u < DST_NOUT; ++u) {
      const uint32_t j = j0 + u * JG;
      if (live && j < L) col[(size_t)j * lstride] = best[u] <= r2 ? best[u] : DST_INF;
    }
  }
}

// the 64 values of word z of brick b as the bits { D2 <= r2 } (a stored value above the cap is +inf already; an empty source
// set leaves +inf everywhere, which is in no ball, whatever r2)
VXD uint64_t dst_word_bits(const float* __restrict__ field, uint32_t b, uint32_t z, uint32_t bc0, uint32_t bc1, float r2) {
  const uint32_t bx = b % bc0, t = b / bc0, by = t % bc1, bz = t / bc1;
  const size_t X = (size_t)bc0 * 8u, Y = (size_t)bc1 * 8u;
  const float* row0 = field + (((size_t)bz * 8u + z) * Y + (size_t)by * 8u) * X + (size_t)bx * 8u;
  uint64_t w = 0;
#pragma unroll
  for (uint32_t y = 0; y < 8u; ++y) {
    const float4* q = reinterpret_cast<const float4*>(row0 + (size_t)y * X);
    const float4 a = q[0], c = q[1];
    const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
    for (uint32_t x = 0; x < 8u; ++x) w |= (uint64_t)(v[x] <= r2 && v[x] < DST_INF ? 1u : 0u) << (y * 8u + x);
  }
  return w;
}

// compare and pack, one lane per word.  shrink = 0: dst = { D2 <= r2 }, with pred (band): dst | (that & pred), dst being the
// segment the field was measured from.  shrink = 1: dst = the complement of { D2 <= r2 }, D2 the distance to the complement of
// the segment: exactly its voxels further than the radius from every voxel outside it.  The lane reads its own word of dst
// before it writes it; no other lane touches that word.
__global__ __launch_bounds__(256) void dst_pack(const float* __restrict__ field, uint64_t* __restrict__ dst,
                                                const uint64_t* __restrict__ pred, const uint32_t shrink, const uint32_t bc0,
                                                const uint32_t bc1, const uint32_t bc2, const float r2) {
  const size_t n = (size_t)bc0 * bc1 * bc2 * 8u, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint64_t in = dst_word_bits(field, (uint32_t)(k >> 3), (uint32_t)(k & 7u), bc0, bc1, r2);
    uint64_t w = shrink ? ~in : in;
    if (pred) w = dst[k] | (w & pred[k]);
    dst[k] = w;
  }
}

VXD void dst_merge(DstPartial& a, const DstPartial& b) {
  a.finite += b.finite;
  if (b.idx != DST_NONE && (a.idx == DST_NONE || b.d2 > a.d2 || (b.d2 == a.d2 && b.idx < a.idx))) {
    a.d2 = b.d2;
    a.idx = b.idx;
  }
}

// the tree of a 256-lane workgroup over LDS; lane 0 ends with the whole
VXD DstPartial dst_block_merge(DstPartial p, DstPartial* sh) {
  sh[threadIdx.x] = p;
  __syncthreads();
  for (uint32_t h = 128u; h > 0u; h >>= 1) {
    if (threadIdx.x < h) dst_merge(sh[threadIdx.x], sh[threadIdx.x + h]);
    __syncthreads();
  }
  return sh[0];
}

// one lane per word of the source mask (complemented by inv): its 64 voxels into a partial; one partial per workgroup
__global__ __launch_bounds__(256) void dst_reduce(const float* __restrict__ field, const uint64_t* __restrict__ mask,
                                                  const uint64_t inv, const uint32_t bc0, const uint32_t bc1, const uint32_t bc2,
                                                  const float r2, DstPartial* __restrict__ partials) {
  __shared__ DstPartial sh[256];
  const size_t n = (size_t)bc0 * bc1 * bc2 * 8u, stride = (size_t)gridDim.x * blockDim.x;
  const size_t X = (size_t)bc0 * 8u, Y = (size_t)bc1 * 8u;
  DstPartial p{0ull, DST_NONE, 0.0f, 0u};
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint32_t b = (uint32_t)(k >> 3), z = (uint32_t)(k & 7u);
    const uint32_t bx = b % bc0, t = b / bc0, by = t % bc1, bz = t / bc1;
    const uint64_t src = mask[k] ^ inv;
    const size_t row0 = (((size_t)bz * 8u + z) * Y + (size_t)by * 8u) * X + (size_t)bx * 8u;
    for (uint32_t y = 0; y < 8u; ++y) {
      const float4* q = reinterpret_cast<const float4*>(field + row0 + (size_t)y * X);
      const float4 a = q[0], c = q[1];
      const float v[8] = {a.x, a.y, a.z, a.w, c.x, c.y, c.z, c.w};
#pragma unroll
      for (uint32_t x = 0; x < 8u; ++x) {
        if (!(v[x] <= r2 && v[x] < DST_INF)) continue;
        ++p.finite;
        if ((src >> (y * 8u + x)) & 1ull) continue;
        dst_merge(p, DstPartial{0ull, (unsigned long long)(row0 + (size_t)y * X + x), v[x], 0u});
      }
    }
  }
  p = dst_block_merge(p, sh);
  if (threadIdx.x == 0u) partials[blockIdx.x] = p;
}

// one workgroup: the partials of dst_reduce into partials[0]
__global__ __launch_bounds__(256) void dst_reduce_final(DstPartial* __restrict__ partials, const uint32_t count) {
  __shared__ DstPartial sh[256];
  DstPartial p{0ull, DST_NONE, 0.0f, 0u};
  for (uint32_t k = threadIdx.x; k < count; k += 256u) dst_merge(p, partials[k]);
  p = dst_block_merge(p, sh);
  if (threadIdx.x == 0u) partials[0] = p;
}

}  // namespace vx
