// vx_segedit.hpp -- edits of the current segment (vx_segment_edit, vx_segment_write_mask; DESIGN.md section 2 "Segment edits"):
// dilate, erode, open, close and fill holes on the brick-major bit masks of vx_segment.hpp, and the upload of a dense mask.
//
//   sed_step<CONN, BAND>   one morphological step, one lane per brick: the brick's 8 words and the facing boundary layers of its
//                          6 / 26 neighbours (seg_incoming) from a SOURCE mask, the result into a DIFFERENT destination mask.
//                          `inv` = ~0 complements every word read and the word written: erode = the dilation of the complement,
//                          where a neighbour outside the volume contributes nothing (it counts as set).  BAND keeps the source
//                          and adds only voxels of the predicate words.  A step never runs in place: another workgroup may
//                          already have advanced a neighbour, and the result is exact, not "eventually".
//   sed_reset              one lane: the statistics' start values (and, with `all`, the rounds, visits and worklist lengths).
//   sed_fill_seed          fill holes, the start of the background flood: predicate = the complement of the mask, the reached
//                          set pre-seeded with the background voxels on the six faces of the volume, the first worklist = the
//                          volume's boundary bricks that hold background.  seg_flood<CONN> runs on this view unchanged.
//   sed_fill_finish        the filled mask = the complement of the reached background.
//   sed_unpack             seg_pack in reverse: the dense packed mask into brick-major words.
// The discipline of vx_segment.hpp holds: plain vector loads and stores, one writer per destination brick per launch, no spin,
// no grid barrier, no cooperative or persistent launch.
#pragma once

#include "vx_segment.hpp"

namespace vx {

VXD void sed_load8(const uint64_t* __restrict__ p, uint64_t inv, uint64_t (&w)[8]) {
  const ulonglong2* q = reinterpret_cast<const ulonglong2*>(p);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const ulonglong2 a = q[k];
    w[2 * k] = a.x ^ inv;
    w[2 * k + 1] = a.y ^ inv;
  }
}

// dst = step(src): all three masks are nb * 8 words; pred is read with BAND only.  src != dst (the host never passes the same).
template <int CONN, bool BAND>
__global__ __launch_bounds__(256) void sed_step(const uint64_t* __restrict__ src, uint64_t* __restrict__ dst,
                                                const uint64_t* __restrict__ pred, const uint64_t inv, const uint32_t bc0,
                                                const uint32_t bc1, const uint32_t bc2) {
  const uint32_t nb = bc0 * bc1 * bc2;
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < nb; b += stride) {
    const uint32_t bx = b % bc0, t = b / bc0, by = t % bc1, bz = t / bc1;
    uint64_t S[8], IN[8], T[8];
    sed_load8(src + (size_t)b * 8u, inv, S);
#pragma unroll
    for (int z = 0; z < 8; ++z) IN[z] = 0ull;
    seg_for_dirs<CONN>([&](auto dx, auto dy, auto dz, auto) {
      constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value, DZ = decltype(dz)::value;
      const bool ok = (DX >= 0 || bx > 0) && (DX <= 0 || bx + 1u < bc0) && (DY >= 0 || by > 0) && (DY <= 0 || by + 1u < bc1) &&
                      (DZ >= 0 || bz > 0) && (DZ <= 0 || bz + 1u < bc2);
      if (ok) {
        // the neighbour's words in registers (complemented for erode), then seg_incoming on that copy: only the facing word of
        // a neighbour above or below is read
        const uint64_t* w = src + (size_t)(b + DX + DY * (int)bc0 + DZ * (int)(bc0 * bc1)) * 8u;
        uint64_t W[8];
        if (DZ != 0) {
#pragma unroll
          for (int z = 0; z < 8; ++z) W[z] = 0ull;
          W[DZ < 0 ? 7 : 0] = w[DZ < 0 ? 7 : 0] ^ inv;
        } else {
          sed_load8(w, inv, W);
        }
        seg_incoming<CONN, DX, DY, DZ>(W, 0u, IN);
      }
    });
    seg_step<CONN>(S, T);
#pragma unroll
    for (int z = 0; z < 8; ++z) T[z] |= IN[z];
    if (BAND) {
      uint64_t P[8];
      sed_load8(pred + (size_t)b * 8u, 0ull, P);
#pragma unroll
      for (int z = 0; z < 8; ++z) T[z] = S[z] | (T[z] & P[z]);
    }
    ulonglong2* o = reinterpret_cast<ulonglong2*>(dst + (size_t)b * 8u);
#pragma unroll
    for (int k = 0; k < 4; ++k) o[k] = make_ulonglong2(T[2 * k] ^ inv, T[2 * k + 1] ^ inv);
  }
}

// one lane: what seg_seed does for the statistics; all != 0 also clears the flood's bookkeeping and the worklist lengths
__global__ void sed_reset(const SegDev s, uint32_t all) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  SegStats* st = s.st;
  st->count = 0;
  for (int a = 0; a < 3; ++a) {
    st->lo[a] = 0xffffffffu;
    st->hi[a] = 0u;
  }
  st->dmin = 0xffffffffu;
  st->dmax = 0u;
  st->sum = 0.0;
  st->pad = 0u;
  if (all) {
    st->rounds = 0u;
    st->visits = 0;
    s.cnt[0] = 0u;
    s.cnt[1] = 0u;
    s.cnt[2] = 0u;
  }
}

// one lane per brick.  f is the flood's view: f.pred = ~mask, f.seg = the background voxels on the volume's faces, f.any, a
// cleared stamp, and the brick appended to round 0's worklist when it lies on the boundary of the brick grid and holds
// background.  (Every boundary brick with background goes in, seeded or not: under 26 a background voxel one layer inside can
// touch a face voxel of the brick beside it only across an edge, and seg_flood appends a neighbour only for GROWN bits.)
// sed_reset(all) ran before: cnt[0] = 0.
__global__ __launch_bounds__(256) void sed_fill_seed(const uint64_t* __restrict__ mask, const SegDev f) {
  const uint32_t stride = gridDim.x * blockDim.x;
  for (uint32_t b = blockIdx.x * blockDim.x + threadIdx.x; b < f.nb; b += stride) {
    const uint32_t bx = b % f.bc[0], t = b / f.bc[0], by = t % f.bc[1], bz = t / f.bc[1];
    uint64_t P[8], any = 0;
    sed_load8(mask + (size_t)b * 8u, ~0ull, P);
    uint64_t face = 0;   // the face voxels of every z slice of this brick
    if (bx == 0u) face |= SEG_COL0;
    if (bx + 1u == f.bc[0]) face |= SEG_COL7;
    if (by == 0u) face |= SEG_ROW0;
    if (by + 1u == f.bc[1]) face |= SEG_ROW7;
    uint64_t R[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      any |= P[z];
      const bool zface = (z == 0 && bz == 0u) || (z == 7 && bz + 1u == f.bc[2]);
      R[z] = P[z] & (zface ? ~0ull : face);
    }
    ulonglong2* po = reinterpret_cast<ulonglong2*>(f.pred + (size_t)b * 8u);
    ulonglong2* ro = reinterpret_cast<ulonglong2*>(f.seg + (size_t)b * 8u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      po[k] = make_ulonglong2(P[2 * k], P[2 * k + 1]);
      ro[k] = make_ulonglong2(R[2 * k], R[2 * k + 1]);
    }
    f.any[b] = any != 0 ? 1u : 0u;
    f.stamp[b] = 0u;
    const bool edge = bx == 0u || by == 0u || bz == 0u || bx + 1u == f.bc[0] || by + 1u == f.bc[1] || bz + 1u == f.bc[2];
    if (edge && any != 0) {
      const uint32_t at = atomicAdd(f.cnt, 1u);
      if (at < f.nb) f.list[0][at] = b;
    }
  }
}

// mask = ~reached over n words: the mask's own voxels were never reached (the flood's predicate excludes them) and stay
__global__ __launch_bounds__(256) void sed_fill_finish(const uint64_t* __restrict__ reached, uint64_t* __restrict__ mask, size_t n) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) mask[k] = ~reached[k];
}

// seg_pack in reverse: word z of brick b gathers byte (z, y, bx) of the dense mask for its 8 rows y.  in holds X * Y * Z / 8
// bytes with X, Y, Z = 8 x bc, so every byte index is inside it.
__global__ __launch_bounds__(256) void sed_unpack(const SegDev s, uint32_t Y, const uint8_t* __restrict__ in) {
  const size_t n = (size_t)s.nb * 8u, stride = (size_t)gridDim.x * blockDim.x;
  const uint32_t rx = s.bc[0];
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint32_t b = (uint32_t)(k >> 3), z = (uint32_t)(k & 7u);
    const uint32_t bx = b % s.bc[0], t = b / s.bc[0], by = t % s.bc[1], bz = t / s.bc[1];
    const size_t row0 = ((size_t)(bz * 8u + z) * Y + by * 8u) * rx + bx;
    uint64_t w = 0;
#pragma unroll
    for (uint32_t y = 0; y < 8u; ++y) w |= (uint64_t)in[row0 + (size_t)y * rx] << (y * 8u);
    s.seg[k] = w;
  }
}

}  // namespace vx
