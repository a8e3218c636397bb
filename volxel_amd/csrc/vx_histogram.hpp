// vx_histogram.hpp -- the kernels of vx_histogram (DESIGN.md section 2 "Histograms"): the density histogram, the moments and the
// radix passes of the order statistics of a region R.  The contract (include/volxel_hip.h "histograms"):
//
//   R        the voxels of index_extent inside the inclusive voxel box that the source selects: every voxel of the box
//            (HstParams::mask == nullptr), or the bits of a brick-major mask of vx_segment.hpp (the current segment or a slot).
//   d(i)     seg_density<LAYOUT>: the density vx_segment thresholds, the same bits on every layout.
//   LINEAR   d < lo: below; d > hi: above; otherwise bin = min(B - 1, (uint32_t)fl32(fl32(d - lo) * inv)), inv = fl32(fl32(B) /
//            fl32(hi - lo)) computed once by the host.  __fsub_rn / __fmul_rn: two roundings, never contracted.  Both are
//            monotone in d -- rounding to nearest keeps the order of the exact differences, and of their exact products with
//            the positive inv -- so bins are monotone in d and cumulative counts are meaningful; d == hi lands in bin B - 1.
//   KEY      key = seg_order_key(d); top = p ? key >> (32 - p) : 0; top < prefix: below; top > prefix: above; otherwise
//            bin = (key >> (32 - p - b)) & (2^b - 1).  Three passes of 11, 11 and 10 bits are a radix select.
//   moments  the float64 sums of (double)d and (double)d * (double)d and the extremes of d over ALL of R, in a fixed order: per
//            brick the order of seg_stats (a lane adds its voxels z = 0 .. 7, then the xor butterfly over the wave) into
//            HstPartial[b], then hst_moments adds the bricks in the tree of seg_sum.  Same bytes on every run, and the sum of a
//            segment is bit for bit the one seg_stats / seg_sum report.
//
//   hst_bins<LAYOUT, MASKED, MOMENTS>   one wave per brick in a grid-stride loop, lane = y * 8 + x, eight z slices: the
//            loop of seg_predicate / seg_stats.  A brick wholly outside the box, or (MASKED) whose eight mask words are all
//            zero, is skipped without touching its voxels.  Bins live in LDS as 32-bit counters -- one copy per wave up to
//            HST_PRIVATE_MAX bins, one per workgroup beyond -- with `below` and `above` as two more counters behind them, and
//            are updated by LDS integer atomics.  Each workgroup adds its non-zero counters once, at its end, to the 64-bit
//            global array the host zeroed, with 64-bit global atomics.  Integer adds commute: the counts are exact and the same
//            on every run, whatever the grid.
//            A lane issues its eight loads before it bins the first, so none waits for another.
//            The rule and the mask source are wave uniform.  A shortcut for z slices whose selected lanes all share one bin
//            (one ballot against the first selected lane's bin, then one LDS add of the popcount) was built and measured: it
//            took 0.70 of the time on the CT phantom and 1.02 - 1.07 of it on spread densities, more than run-to-run noise, and
//            was taken out again (NOTEBOOK "Histograms").
//   hst_moments   one workgroup of 1024: the bricks' partials into one.
// No 32-bit LDS counter can wrap before its flush: a workgroup counts at most 512 voxels for each brick it visits, it visits
// at most 4 * ceil(nb / (4 * grid)) bricks, the host launches min(ceil(nb / 4), HST_MAX_BLOCKS = 1024) workgroups and nb < 2^32,
// so a workgroup counts fewer than 512 * (2^22 + 4) < 2^32 voxels in all its counters together.
// The discipline of vx_segment.hpp holds: no cross-workgroup hand-off inside a launch (no spin, no grid barrier, no cooperative
// or persistent launch); the zeroing, the histogram and the moments' tree are separated by kernel boundaries; results leave
// through plain vector stores and vector atomics.
#pragma once

#include "vx_segment.hpp"

namespace vx {

constexpr uint32_t HST_PRIVATE_MAX = 1024u;                      // bins up to which each of the 4 waves has its own copy
constexpr uint32_t HST_LDS_WORDS = 4u * (HST_PRIVATE_MAX + 2u);   // 4104 >= VX_HIST_MAX_BINS + 2: 16 KiB of LDS
constexpr uint32_t HST_MAX_BLOCKS = 1024u;
static_assert(HST_LDS_WORDS >= VX_HIST_MAX_BINS + 2u && (1u << VX_HIST_MAX_KEY_BITS) <= VX_HIST_MAX_BINS, "the LDS holds every legal bin count");

// the counter of density d: its bin, h.bins for `below`, h.bins + 1 for `above` (wave-uniform branch on the rule)
VXD uint32_t hst_bin(const HstParams& h, float d) {
  if (h.rule == VX_HIST_LINEAR) {
    if (d < h.lo) return h.bins;
    if (d > h.hi) return h.bins + 1u;
    return min(h.bins - 1u, (uint32_t)__fmul_rn(__fsub_rn(d, h.lo), h.inv));
  }
  const uint32_t key = seg_order_key(d);
  const uint32_t top = h.top_shift < 32u ? key >> h.top_shift : 0u;
  if (top < h.prefix) return h.bins;
  if (top > h.prefix) return h.bins + 1u;
  return (key >> h.bin_shift) & h.bin_mask;
}

template <int LAYOUT, bool MASKED, bool MOMENTS>
__global__ __launch_bounds__(256) void hst_bins(const DevVolume v, float scale, float inv_maj, const HstParams h) {
  __shared__ uint32_t sh[HST_LDS_WORDS];
  const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3, wave = threadIdx.x >> 6;
  const uint32_t slots = h.bins + 2u;                               // the bins, below, above
  const uint32_t copies = h.bins <= HST_PRIVATE_MAX ? 4u : 1u;       // copies * slots <= HST_LDS_WORDS
  for (uint32_t i = threadIdx.x; i < slots * copies; i += 256u) sh[i] = 0u;
  __syncthreads();
  uint32_t* mine = sh + (copies == 4u ? wave * slots : 0u);
  const float inf = __int_as_float(0x7f800000);
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = blockIdx.x * 4u + wave; b < h.nb; b += waves) {   // wave uniform
    const uint32_t bx = b % h.bc[0], t = b / h.bc[0], by = t % h.bc[1], bz = t / h.bc[1];
    const bool outside = bx * 8u + 7u < h.box_lo[0] || bx * 8u > h.box_hi[0] || by * 8u + 7u < h.box_lo[1] || by * 8u > h.box_hi[1] ||
                         bz * 8u + 7u < h.box_lo[2] || bz * 8u > h.box_hi[2];
    uint64_t S[8], u = 0;
    if (!outside) {
      if (MASKED) {
        const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(h.mask + (size_t)b * 8u);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const ulonglong2 a = sp[k];
          S[2 * k] = a.x;
          S[2 * k + 1] = a.y;
          u |= a.x | a.y;
        }
      } else {
#pragma unroll
        for (int k = 0; k < 8; ++k) S[k] = ~0ull;
        u = ~0ull;
      }
    }
    if (!u) {   // outside the box, or no bit of the mask: no voxel is read
      if (MOMENTS && lane == 0u) h.partial[b] = HstPartial{0.0, 0.0, inf, -inf};
      continue;
    }
    const uint32_t x = bx * 8u + lx, y = by * 8u + ly;
    // no brick is partial: vx_upload_volume requires index_extent = 8 x the brick grid, and the box lies inside it
    const bool in_xy = x >= h.box_lo[0] && x <= h.box_hi[0] && y >= h.box_lo[1] && y <= h.box_hi[1];
    // the eight loads of a lane first, none waiting for another: the slices' bins and atomics follow when they have arrived
    float dv[8];
    uint64_t M[8];
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      const uint32_t zz = bz * 8u + z;
      const bool sel = in_xy && zz >= h.box_lo[2] && zz <= h.box_hi[2] && ((S[z] >> lane) & 1ull);
      M[z] = __ballot(sel);
      dv[z] = sel ? seg_density<LAYOUT>(v, scale, inv_maj, x, y, zz) : 0.0f;
    }
    double sum = 0.0, sum2 = 0.0;
    float mn = inf, mx = -inf;
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      const uint64_t m = M[z];
      if (m == 0ull) continue;   // wave uniform
      const bool sel = (m >> lane) & 1ull;
      uint32_t bin = 0xffffffffu;
      if (sel) {
        const float d = dv[z];
        bin = hst_bin(h, d);
        if (MOMENTS) {
          const double dd = (double)d;
          sum += dd;
          sum2 += dd * dd;
          mn = fminf(mn, d);
          mx = fmaxf(mx, d);
        }
      }
      if (sel) atomicAdd(mine + bin, 1u);
    }
    if (MOMENTS) {
#pragma unroll
      for (int o = 1; o < 64; o <<= 1) {
        sum += __shfl_xor(sum, o);
        sum2 += __shfl_xor(sum2, o);
        mn = fminf(mn, __shfl_xor(mn, o));
        mx = fmaxf(mx, __shfl_xor(mx, o));
      }
      if (lane == 0u) h.partial[b] = HstPartial{sum, sum2, mn, mx};
    }
  }
  __syncthreads();
  for (uint32_t i = threadIdx.x; i < slots; i += 256u) {
    uint32_t n = 0;
    for (uint32_t k = 0; k < copies; ++k) n += sh[k * slots + i];
    if (n) atomicAdd(h.out + i, (unsigned long long)n);
  }
}

// one workgroup of 1024: thread t merges bricks [t * chunk, (t + 1) * chunk) in order, then the fixed tree of seg_sum in LDS
__global__ __launch_bounds__(1024) void hst_moments(const HstPartial* __restrict__ partial, const uint32_t nb, HstPartial* __restrict__ out) {
  __shared__ HstPartial part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (nb + 1023u) / 1024u;
  const uint32_t b0 = min(nb, t * chunk), b1 = min(nb, b0 + chunk);
  HstPartial a{0.0, 0.0, __int_as_float(0x7f800000), -__int_as_float(0x7f800000)};
  for (uint32_t b = b0; b < b1; ++b) {
    const HstPartial p = partial[b];
    a.sum += p.sum;
    a.sum2 += p.sum2;
    a.mn = fminf(a.mn, p.mn);
    a.mx = fmaxf(a.mx, p.mx);
  }
  part[t] = a;
  __syncthreads();
  for (uint32_t s = 512u; s > 0u; s >>= 1) {
    if (t < s) {
      part[t].sum += part[t + s].sum;
      part[t].sum2 += part[t + s].sum2;
      part[t].mn = fminf(part[t].mn, part[t + s].mn);
      part[t].mx = fmaxf(part[t].mx, part[t + s].mx);
    }
    __syncthreads();
  }
  if (t == 0u) *out = part[0];
}

}  // namespace vx
