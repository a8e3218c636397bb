// vx_segment.hpp -- seeded region growing (vx_segment, DESIGN.md section 2 "Segmentation"): the connected component of the
// predicate lo <= d(i) <= hi (inside a voxel box) that holds the seed, as bit masks over the 8^3 bricks of the brick grid.
//
// Masks are brick-major: brick b (x fastest over indirection_size) is 8 x u64, word z, bit y * 8 + x.
//   seg_predicate<LAYOUT>  one wave per brick, lane = y * 8 + x, one ballot per z slice: the predicate words and a per-brick
//                          "any bit" flag.
//   seg_seed               one lane: the first worklist (the seed's brick when P(seed)) and the statistics' start values.
//   seg_flood<CONN>        one round: one lane per worklist brick.  It ORs in the neighbours' boundary bits, dilates inside the
//                          brick to a fixpoint (64-bit shifts and masks), stores the brick when it changed, and appends the
//                          neighbours whose facing boundary grew to the next worklist.
//   seg_stats<LAYOUT>      one wave per brick: count, bbox and min / max by atomics on order-preserving integers, and the
//                          brick's float64 sum in a fixed order into a per-brick buffer; seg_sum adds those in a fixed tree.
//   seg_pack / seg_slice_mask   the dense packed mask and the slice overlay.
// Coherence: a round reads its neighbours' words with plain loads, possibly stale within the launch.  Bits are only ever set,
// and every new boundary bit appends its neighbour to the next round, which starts after the kernel boundary: stale reads cost
// a round, never a bit.  No spin, no grid barrier, no persistent or cooperative launch; masks are written with plain vector
// stores, one writer per brick per launch (a brick is in a worklist at most once: the stamp).
#pragma once

#include "vx_slice.hpp"

namespace vx {

constexpr uint32_t SEG_FIXPOINT_MAX = 512u;   // in-brick dilation steps: each one that changes adds a voxel

// the seed of the flood: its brick, word and bit
struct SegSeed {
  uint32_t b, z;
  uint64_t bit;
};

// a float's bits as an unsigned key with the float order (-0 below +0)
VXD uint32_t seg_order_key(float f) {
  const uint32_t u = __float_as_uint(f);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

struct SegPredParams {
  float lo, hi;
  uint32_t box_lo[3], box_hi[3];
};

template <int LAYOUT>
__global__ __launch_bounds__(256) void seg_predicate(const DevVolume v, float scale, float inv_maj, const SegPredParams pp,
                                                     const SegDev s) {
  const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6); b < s.nb; b += waves) {   // wave uniform
    const uint32_t bx = b % s.bc[0], t = b / s.bc[0], by = t % s.bc[1], bz = t / s.bc[1];
    const uint32_t x = bx * 8u + lx, y = by * 8u + ly;
    // no brick is partial: vx_upload_volume requires index_extent = 8 x the brick grid, and the box lies inside it
    const bool in_xy = x >= pp.box_lo[0] && x <= pp.box_hi[0] && y >= pp.box_lo[1] && y <= pp.box_hi[1];
    uint64_t mine = 0, any = 0;
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      const uint32_t zz = bz * 8u + z;
      const float d = seg_density<LAYOUT>(v, scale, inv_maj, x, y, zz);
      const bool p = in_xy && zz >= pp.box_lo[2] && zz <= pp.box_hi[2] && pp.lo <= d && d <= pp.hi;
      const uint64_t w = __ballot(p);
      mine = lane == z ? w : mine;
      any |= w;
    }
    if (lane < 8u) s.pred[(size_t)b * 8u + lane] = mine;
    if (lane == 0u) s.any[b] = any != 0 ? 1u : 0u;
  }
}

// one lane: the statistics' start values and round 0's worklist (the seed's brick when its predicate bit is set)
__global__ void seg_seed(const SegDev s, const SegSeed seed) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  const bool on = (s.pred[(size_t)seed.b * 8u + seed.z] & seed.bit) != 0;
  s.list[0][0] = seed.b;
  s.cnt[0] = on ? 1u : 0u;
  s.cnt[1] = 0u;
  s.cnt[2] = 0u;
  SegStats* st = s.st;
  st->count = 0;
  for (int a = 0; a < 3; ++a) {
    st->lo[a] = 0xffffffffu;
    st->hi[a] = 0u;
  }
  st->dmin = 0xffffffffu;
  st->dmax = 0u;
  st->sum = 0.0;
  st->rounds = 0u;
  st->pad = 0u;
  st->visits = 0;
}

// the boundary layer of a neighbour at (dx, dy) in the plane, moved across the shared face / edge into this brick's layer
template <int DX, int DY>
VXD uint64_t seg_place(uint64_t w) {
  if (DX < 0) w = (w & SEG_COL7) >> 7;
  else if (DX > 0) w = (w & SEG_COL0) << 7;
  if (DY < 0) w = (w & SEG_ROW7) >> 56;
  else if (DY > 0) w = (w & SEG_ROW0) << 56;
  return w;
}
VXD uint64_t seg_dil_x(uint64_t w) { return w | ((w & ~SEG_COL7) << 1) | ((w & ~SEG_COL0) >> 1); }
VXD uint64_t seg_dil_y(uint64_t w) { return w | (w << 8) | (w >> 8); }

// the bits the neighbour at (DX, DY, DZ) -- brick nb -- reaches in this brick: its facing boundary moved across, then for 26
// dilated along the axes where it lies level with this brick (the 3x3x3 box is separable)
template <int CONN, int DX, int DY, int DZ>
VXD void seg_incoming(const uint64_t* __restrict__ seg, uint32_t nb, uint64_t (&in)[8]) {
  const uint64_t* w = seg + (size_t)nb * 8u;
  if (DZ != 0) {
    uint64_t t = seg_place<DX, DY>(w[DZ < 0 ? 7 : 0]);
    if (CONN == 26 && DX == 0) t = seg_dil_x(t);
    if (CONN == 26 && DY == 0) t = seg_dil_y(t);
    in[DZ < 0 ? 0 : 7] |= t;
  } else {
    uint64_t t[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      t[z] = seg_place<DX, DY>(w[z]);
      if (CONN == 26 && DX == 0) t[z] = seg_dil_x(t[z]);
      if (CONN == 26 && DY == 0) t[z] = seg_dil_y(t[z]);
    }
#pragma unroll
    for (int z = 0; z < 8; ++z) in[z] |= (CONN == 26) ? (t[z] | (z > 0 ? t[z - 1] : 0) | (z < 7 ? t[z + 1] : 0)) : t[z];
  }
}

// the boundary region of this brick that faces the neighbour at (DX, DY, DZ), as the OR of the grown bits there
template <int DX, int DY, int DZ>
VXD bool seg_faces(const uint64_t (&g)[8]) {
  uint64_t w = 0;
  if (DZ < 0) w = g[0];
  else if (DZ > 0) w = g[7];
  else
#pragma unroll
    for (int z = 0; z < 8; ++z) w |= g[z];
  if (DX < 0) w &= SEG_COL0;
  else if (DX > 0) w &= SEG_COL7;
  if (DY < 0) w &= SEG_ROW0;
  else if (DY > 0) w &= SEG_ROW7;
  return w != 0;
}

// calls f(integral_constant DX, DY, DZ, direction index) for the 6 faces, or the 26 neighbours
template <int CONN, int D = 0, class F>
VXD void seg_for_dirs(F&& f) {
  if constexpr (D < 27) {
    constexpr int DX = D % 3 - 1, DY = (D / 3) % 3 - 1, DZ = D / 9 - 1;
    constexpr int NZ = (DX != 0) + (DY != 0) + (DZ != 0);
    if constexpr (NZ != 0 && (CONN == 26 || NZ == 1))
      f(std::integral_constant<int, DX>{}, std::integral_constant<int, DY>{}, std::integral_constant<int, DZ>{},
        std::integral_constant<int, D>{});
    seg_for_dirs<CONN, D + 1>(f);
  }
}

// one in-brick dilation step: 6 = the faces, 26 = the 3x3x3 box
template <int CONN>
VXD void seg_step(const uint64_t (&s)[8], uint64_t (&t)[8]) {
  uint64_t a[8];
#pragma unroll
  for (int z = 0; z < 8; ++z) a[z] = CONN == 26 ? seg_dil_y(seg_dil_x(s[z])) : s[z];
#pragma unroll
  for (int z = 0; z < 8; ++z) {
    const uint64_t zn = (z > 0 ? a[z - 1] : 0) | (z < 7 ? a[z + 1] : 0);
    t[z] = CONN == 26 ? (a[z] | zn) : (s[z] | ((s[z] & ~SEG_COL7) << 1) | ((s[z] & ~SEG_COL0) >> 1) | (s[z] << 8) | (s[z] >> 8) | zn);
  }
}

// round `round` of the flood: worklist list[round & 1] of cnt[round % 3] bricks; appends go to list[(round + 1) & 1] /
// cnt[(round + 1) % 3]; cnt[(round + 2) % 3] is cleared for the round after (nothing in this launch reads it)
template <int CONN>
__global__ __launch_bounds__(256) void seg_flood(const SegDev s, const SegSeed seed, uint32_t round) {
  const uint32_t n = s.cnt[round % 3u];
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    s.cnt[(round + 2u) % 3u] = 0u;
    if (n) {
      s.st->rounds += 1u;
      s.st->visits += n;
    }
  }
  const uint32_t* __restrict__ in_list = s.list[round & 1u];
  uint32_t* __restrict__ out_list = s.list[(round + 1u) & 1u];
  uint32_t* out_cnt = s.cnt + (round + 1u) % 3u;
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t stride = gridDim.x * blockDim.x;
  const uint32_t tag = round + 1u;
  for (uint32_t base = blockIdx.x * blockDim.x + (threadIdx.x & ~63u); base < n; base += stride) {   // wave uniform
    const uint32_t i = base + lane;
    uint32_t b = 0, wins = 0;
    uint32_t bx = 0, by = 0, bz = 0;
    if (i < n) {
      b = in_list[i];
      bx = b % s.bc[0];
      const uint32_t t = b / s.bc[0];
      by = t % s.bc[1];
      bz = t / s.bc[1];
      uint64_t P[8], S[8], O[8], IN[8];
      const ulonglong2* pp = reinterpret_cast<const ulonglong2*>(s.pred + (size_t)b * 8u);
      const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(s.seg + (size_t)b * 8u);
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const ulonglong2 a = pp[k], c = sp[k];
        P[2 * k] = a.x;
        P[2 * k + 1] = a.y;
        O[2 * k] = c.x;
        O[2 * k + 1] = c.y;
      }
#pragma unroll
      for (int z = 0; z < 8; ++z) IN[z] = (b == seed.b && (uint32_t)z == seed.z) ? seed.bit : 0ull;
      seg_for_dirs<CONN>([&](auto dx, auto dy, auto dz, auto) {
        constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value, DZ = decltype(dz)::value;
        const bool ok = (DX >= 0 || bx > 0) && (DX <= 0 || bx + 1u < s.bc[0]) && (DY >= 0 || by > 0) && (DY <= 0 || by + 1u < s.bc[1]) &&
                        (DZ >= 0 || bz > 0) && (DZ <= 0 || bz + 1u < s.bc[2]);
        if (ok) seg_incoming<CONN, DX, DY, DZ>(s.seg, b + DX + DY * (int)s.bc[0] + DZ * (int)(s.bc[0] * s.bc[1]), IN);
      });
#pragma unroll
      for (int z = 0; z < 8; ++z) S[z] = O[z] | (IN[z] & P[z]);
      for (uint32_t it = 0; it < SEG_FIXPOINT_MAX; ++it) {
        uint64_t T[8];
        seg_step<CONN>(S, T);
        uint64_t diff = 0;
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          T[z] &= P[z];
          diff |= T[z] ^ S[z];
          S[z] = T[z];
        }
        if (!diff) break;
      }
      uint64_t G[8], grew = 0;
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        G[z] = S[z] & ~O[z];
        grew |= G[z];
      }
      if (grew) {
        ulonglong2* so = reinterpret_cast<ulonglong2*>(s.seg + (size_t)b * 8u);
#pragma unroll
        for (int k = 0; k < 4; ++k) so[k] = make_ulonglong2(S[2 * k], S[2 * k + 1]);
        seg_for_dirs<CONN>([&](auto dx, auto dy, auto dz, auto d) {
          constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value, DZ = decltype(dz)::value, D = decltype(d)::value;
          const bool ok = (DX >= 0 || bx > 0) && (DX <= 0 || bx + 1u < s.bc[0]) && (DY >= 0 || by > 0) &&
                          (DY <= 0 || by + 1u < s.bc[1]) && (DZ >= 0 || bz > 0) && (DZ <= 0 || bz + 1u < s.bc[2]);
          if (ok && seg_faces<DX, DY, DZ>(G)) {
            const uint32_t nbr = b + DX + DY * (int)s.bc[0] + DZ * (int)(s.bc[0] * s.bc[1]);
            if (s.any[nbr] && atomicExch(s.stamp + nbr, tag) != tag) wins |= 1u << D;
          }
        });
      }
    }
    // the wave's appends: one atomic add of their total, each lane's entries at its exclusive prefix
    const uint32_t k = (uint32_t)__popc(wins);
    uint32_t incl = k;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t u = __shfl_up(incl, o);
      incl += lane >= (uint32_t)o ? u : 0u;
    }
    const uint32_t total = __shfl(incl, 63);
    if (total) {
      uint32_t at = 0;
      if (lane == 63u) at = atomicAdd(out_cnt, total);
      at = __shfl(at, 63) + incl - k;
      while (wins) {
        const int D = __ffs(wins) - 1;
        wins &= wins - 1u;
        const int DX = D % 3 - 1, DY = (D / 3) % 3 - 1, DZ = D / 9 - 1;
        if (at < s.nb) out_list[at] = b + DX + DY * (int)s.bc[0] + DZ * (int)(s.bc[0] * s.bc[1]);
        ++at;
      }
    }
  }
}

// one wave per brick: count, bbox, min / max and the brick's float64 sum (voxels in z, y, x order per lane, then a fixed
// butterfly over the wave); a brick without segment bits writes a sum of 0
template <int LAYOUT>
__global__ __launch_bounds__(256) void seg_stats(const DevVolume v, float scale, float inv_maj, const SegDev s) {
  const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6); b < s.nb; b += waves) {   // wave uniform
    uint64_t S[8], u = 0;
    const ulonglong2* sp = reinterpret_cast<const ulonglong2*>(s.seg + (size_t)b * 8u);
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const ulonglong2 a = sp[k];
      S[2 * k] = a.x;
      S[2 * k + 1] = a.y;
      u |= a.x | a.y;
    }
    if (!u) {
      if (lane == 0u) s.partial[b] = 0.0;
      continue;
    }
    const uint32_t bx = b % s.bc[0], t = b / s.bc[0], by = t % s.bc[1], bz = t / s.bc[1];
    double sum = 0.0;
    float mn = __int_as_float(0x7f800000), mx = -__int_as_float(0x7f800000);
    uint32_t cnt = 0, zl = 8, zh = 0;
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      cnt += (uint32_t)__popcll(S[z]);
      if (S[z]) {
        zl = min(zl, z);
        zh = z;
      }
      if ((S[z] >> lane) & 1ull) {
        const float d = seg_density<LAYOUT>(v, scale, inv_maj, bx * 8u + lx, by * 8u + ly, bz * 8u + z);
        sum += (double)d;
        mn = fminf(mn, d);
        mx = fmaxf(mx, d);
      }
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      sum += __shfl_xor(sum, o);
      mn = fminf(mn, __shfl_xor(mn, o));
      mx = fmaxf(mx, __shfl_xor(mx, o));
    }
    if (lane == 0u) {
      uint32_t cols = 0, rows = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint32_t row = (uint32_t)(u >> (8 * r)) & 255u;
        cols |= row;
        rows |= row ? 1u << r : 0u;
      }
      SegStats* st = s.st;
      atomicAdd(&st->count, (unsigned long long)cnt);
      atomicMin(&st->lo[0], bx * 8u + (uint32_t)(__ffs(cols) - 1));
      atomicMax(&st->hi[0], bx * 8u + (uint32_t)(31 - __clz(cols)));
      atomicMin(&st->lo[1], by * 8u + (uint32_t)(__ffs(rows) - 1));
      atomicMax(&st->hi[1], by * 8u + (uint32_t)(31 - __clz(rows)));
      atomicMin(&st->lo[2], bz * 8u + zl);
      atomicMax(&st->hi[2], bz * 8u + zh);
      atomicMin(&st->dmin, seg_order_key(mn));
      atomicMax(&st->dmax, seg_order_key(mx));
      s.partial[b] = sum;
    }
  }
}

// one workgroup of 1024: thread t adds bricks [t * chunk, (t + 1) * chunk) in order, then a fixed tree in LDS
__global__ __launch_bounds__(1024) void seg_sum(const SegDev s) {
  __shared__ double part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (s.nb + 1023u) / 1024u;
  const uint32_t b0 = min(s.nb, t * chunk), b1 = min(s.nb, b0 + chunk);
  double a = 0.0;
  for (uint32_t b = b0; b < b1; ++b) a += s.partial[b];
  part[t] = a;
  __syncthreads();
  for (uint32_t h = 512u; h > 0u; h >>= 1) {
    if (t < h) part[t] += part[t + h];
    __syncthreads();
  }
  if (t == 0u) s.st->sum = part[0];
}

// the dense packed mask: byte k holds voxels 8k .. 8k + 7 of (z, y, x) in C order, LSB first.  X is a multiple of 8
// (vx_upload_volume requires index_extent = 8 x the brick grid), so a byte is one row of one brick: byte y of word z.
__global__ __launch_bounds__(256) void seg_pack(const SegDev s, uint32_t X, uint32_t Y, size_t nbytes, uint8_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  const uint32_t rx = X >> 3;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < nbytes; k += stride) {
    const uint32_t xb = (uint32_t)(k % rx);
    const size_t r = k / rx;
    const uint32_t y = (uint32_t)(r % Y), z = (uint32_t)(r / Y);
    const uint32_t b = ((z >> 3) * s.bc[1] + (y >> 3)) * s.bc[0] + xb;
    out[k] = (uint8_t)(s.seg[(size_t)b * 8u + (z & 7u)] >> ((y & 7u) * 8u));
  }
}

// the slice overlay: pixel (x, y) is 1 when the nearest voxel floor(q + 1/2) of any slab sample lies in the segment.  q is
// slice_reduce's fma chain and clamp; the mapping of pixels to lanes is slice_reduce's.
__global__ __launch_bounds__(256) void seg_slice_mask(const VxSliceParams sp, const SegDev s, uint32_t ex, uint32_t ey, uint32_t ez,
                                                      uint8_t* __restrict__ out) {
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t y = blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  const uint32_t W = sp.size[0], H = sp.size[1];
  if (x >= W || y >= H) return;
  const float fx = (float)x, fy = (float)y;
  const float bx = fma_(fy, sp.dv[0], fma_(fx, sp.du[0], sp.origin[0]));
  const float by = fma_(fy, sp.dv[1], fma_(fx, sp.du[1], sp.origin[1]));
  const float bz = fma_(fy, sp.dv[2], fma_(fx, sp.du[2], sp.origin[2]));
  const float nf = (float)sp.slab_samples;   // <= 4096: exact
  uint32_t hit = 0;
  for (float fs = 0.0f; fs < nf && !hit; fs += 1.0f) {
    const float qx = fminf(fmaxf(fma_(fs, sp.dn[0], bx), -SLICE_Q_MAX), SLICE_Q_MAX);
    const float qy = fminf(fmaxf(fma_(fs, sp.dn[1], by), -SLICE_Q_MAX), SLICE_Q_MAX);
    const float qz = fminf(fmaxf(fma_(fs, sp.dn[2], bz), -SLICE_Q_MAX), SLICE_Q_MAX);
    const int ix = f2i(floorf(qx + 0.5f)), iy = f2i(floorf(qy + 0.5f)), iz = f2i(floorf(qz + 0.5f));
    if ((uint32_t)ix < ex && (uint32_t)iy < ey && (uint32_t)iz < ez) {
      const uint32_t ux = (uint32_t)ix, uy = (uint32_t)iy, uz = (uint32_t)iz;
      const uint32_t b = ((uz >> 3) * s.bc[1] + (uy >> 3)) * s.bc[0] + (ux >> 3);
      hit = (uint32_t)(s.seg[(size_t)b * 8u + (uz & 7u)] >> (((uy & 7u) << 3) | (ux & 7u))) & 1u;
    }
  }
  out[(size_t)y * W + x] = (uint8_t)hit;
}

}  // namespace vx
