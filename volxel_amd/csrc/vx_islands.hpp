// vx_islands.hpp -- the islands of the current segment (vx_segment_islands, DESIGN.md section 2 "Islands"): every 6- / 26-
// connected component of the brick-major bit mask of vx_segment.hpp, labelled by a union-find whose launch count does not depend
// on the mask, a table of the components (count, anchor, bbox) and the ops that keep some of them.
//
// Labels are one u32 per voxel, brick-major: voxel (z, y, x) of brick b is entry b * 512 + z * 64 + y * 8 + x -- its own index.
// While the forest is built an entry of a set voxel is the index of its parent (a root holds its own index; parents only ever
// move to SMALLER indices, so there are no cycles); afterwards it is ISL_ID | the row of its island in the table.
//   isl_local<CONN>    one wave per brick with a bit: peels the brick's in-brick components (lowest set bit, seg_step<CONN> to a
//                      fixpoint under the brick's words -- wave-uniform work), every voxel's entry = the index of its component's
//                      lowest voxel.
//   isl_merge<CONN>    one wave per brick: every set voxel on the brick's boundary looks at the 3 / 13 neighbours of the lower
//                      half of its neighbourhood that lie in ANOTHER brick and unites the two trees (isl_union).  Every pair
//                      of adjacent voxels across a brick boundary is met once, from its higher end.
//   isl_flatten        every set voxel's entry -> its root; the number of roots per brick.
//   isl_scan           one workgroup: the exclusive scan of those counts, their total.
//   isl_rootid         every root gets its row: the brick's offset + its rank among the brick's roots (a ballot prefix; a
//                      function of the mask only), the row's start values, the entry becomes ISL_ID | row.
//   isl_table          every set voxel's entry -> ISL_ID | row; count, anchor and bbox of the rows by integer atomics (order-
//                      free, hence exact), one flush per run of equal rows in a brick and not one per voxel.
//   isl_seed_row       one lane: the row of one voxel (KEEP_AT).
//   isl_apply          the new mask: a voxel stays when its row's new label is not 0.  One writer per brick, in place.
//   isl_labels_out     the dense (Z, Y, X) label volume, on request.
// Coherence inside isl_merge: the forest is read and written by every workgroup of the launch, per-XCD L2s are not coherent and
// a CU's L1 is never refreshed by another CU's stores, so EVERY access to it there is an agent-scope atomic (load, compare-
// exchange, min).  A stale parent would only cost a retry; a union is never lost: the compare-exchange links a tree only while
// its root still is one, and a failed one starts again from the new roots.  The retry loop makes progress on its own -- nothing
// waits for another workgroup; no fence, flag, grid barrier, cooperative or persistent launch.  The other kernels read what an
// EARLIER launch wrote with plain loads; where isl_flatten / isl_table overwrite an entry another lane may be walking through,
// both the old and the new value are ancestors (or the row) of the same tree.
#pragma once

#include "vx_segedit.hpp"

namespace vx {

constexpr uint32_t ISL_NONE = 0xffffffffu;   // the entry of an unset voxel (never followed: the mask bit is tested first)
constexpr uint32_t ISL_ID = 0x80000000u;     // an entry that holds a table row; voxel indices and rows stay below 2^31

#define ISL_RLX_AGENT __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT

// the root of x; the start node is moved up to it (a min: parents only decrease, and the root is an ancestor)
VXD uint32_t isl_find(uint32_t* p, uint32_t x) {
  const uint32_t x0 = x;
  uint32_t q = __hip_atomic_load(p + x, ISL_RLX_AGENT);
  const uint32_t q0 = q;
  while (q != x) {
    x = q;
    q = __hip_atomic_load(p + x, ISL_RLX_AGENT);
  }
  if (x != q0) __hip_atomic_fetch_min(p + x0, x, ISL_RLX_AGENT);
  return x;
}

// unites the trees of a and b: the larger root is linked under the smaller one while it still is a root
VXD void isl_union(uint32_t* p, uint32_t a, uint32_t b, uint32_t* retries) {
  for (;;) {
    a = isl_find(p, a);
    b = isl_find(p, b);
    if (a == b) return;
    if (a < b) {
      const uint32_t t = a;
      a = b;
      b = t;
    }
    uint32_t expect = a;
    if (__hip_atomic_compare_exchange_strong(p + a, &expect, b, __ATOMIC_RELAXED, ISL_RLX_AGENT)) return;
    __hip_atomic_fetch_add(retries, 1u, ISL_RLX_AGENT);
  }
}

// the first brick of this wave (4 waves per workgroup), in a scalar register: the brick's words and the peel are wave uniform
VXD uint32_t isl_wave_brick() { return (uint32_t)__builtin_amdgcn_readfirstlane((int)(blockIdx.x * 4u + (threadIdx.x >> 6))); }

VXD bool isl_load_brick(const uint64_t* __restrict__ seg, uint32_t b, uint64_t (&M)[8]) {
  sed_load8(seg + (size_t)b * 8u, 0ull, M);
  uint64_t u = 0;
#pragma unroll
  for (int z = 0; z < 8; ++z) u |= M[z];
  return u != 0;
}

template <int CONN>
__global__ __launch_bounds__(256) void isl_local(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    uint64_t R[8];
    if (!isl_load_brick(s.seg, b, R)) continue;
    uint32_t L[8];
#pragma unroll
    for (int z = 0; z < 8; ++z) L[z] = ISL_NONE;
    // at most 256 components (6) / 64 (26) in a brick; each peel removes at least one voxel
    for (uint32_t comp = 0; comp < 512u; ++comp) {
      uint32_t zz = 8u;
      uint64_t w = 0;
#pragma unroll
      for (int z = 7; z >= 0; --z)
        if (R[z]) {
          zz = (uint32_t)z;
          w = R[z];
        }
      if (zz == 8u) break;
      const uint32_t bit = (uint32_t)__ffsll((unsigned long long)w) - 1u;
      const uint32_t root = b * 512u + zz * 64u + bit;
      uint64_t S[8];
#pragma unroll
      for (int z = 0; z < 8; ++z) S[z] = (uint32_t)z == zz ? 1ull << bit : 0ull;
      for (uint32_t it = 0; it < SEG_FIXPOINT_MAX; ++it) {
        uint64_t T[8];
        seg_step<CONN>(S, T);
        uint64_t diff = 0;
#pragma unroll
        for (int z = 0; z < 8; ++z) {
          T[z] &= R[z];
          diff |= T[z] ^ S[z];
          S[z] = T[z];
        }
        if (!diff) break;
      }
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        if ((S[z] >> lane) & 1ull) L[z] = root;
        R[z] &= ~S[z];
      }
    }
    uint32_t* o = d.lab + (size_t)b * 512u + lane;
#pragma unroll
    for (int z = 0; z < 8; ++z) o[z * 64] = L[z];
  }
}

template <int CONN>
__global__ __launch_bounds__(256) void isl_merge(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
  const uint32_t waves = gridDim.x * 4u;
  const int EX = (int)(s.bc[0] * 8u), EY = (int)(s.bc[1] * 8u), EZ = (int)(s.bc[2] * 8u);
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    uint64_t M[8];
    if (!isl_load_brick(s.seg, b, M)) continue;
    const uint32_t bx = b % s.bc[0], t = b / s.bc[0], by = t % s.bc[1], bz = t / s.bc[1];
    const bool edge_xy = lx == 0 || lx == 7 || ly == 0 || ly == 7;
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      if (!((M[z] >> lane) & 1ull) || !(edge_xy || z == 0 || z == 7)) continue;
      const uint32_t me = b * 512u + (uint32_t)z * 64u + lane;
      seg_for_dirs<CONN>([&](auto dx, auto dy, auto dz, auto dd) {
        constexpr int DX = decltype(dx)::value, DY = decltype(dy)::value, DZ = decltype(dz)::value, D = decltype(dd)::value;
        if constexpr (D < 13) {   // the lower half: (DZ, DY, DX) lexicographically below 0
          const int nx = lx + DX, ny = ly + DY, nz = z + DZ;
          if (((nx | ny | nz) & ~7) != 0) {   // in another brick
            const int gx = (int)(bx * 8u) + nx, gy = (int)(by * 8u) + ny, gz = (int)(bz * 8u) + nz;
            if (gx >= 0 && gx < EX && gy >= 0 && gy < EY && gz >= 0 && gz < EZ) {
              const uint32_t ob = (((uint32_t)gz >> 3) * s.bc[1] + ((uint32_t)gy >> 3)) * s.bc[0] + ((uint32_t)gx >> 3);
              const uint32_t obit = (((uint32_t)gy & 7u) << 3) | ((uint32_t)gx & 7u);
              if ((s.seg[(size_t)ob * 8u + ((uint32_t)gz & 7u)] >> obit) & 1ull)
                isl_union(d.lab, me, ob * 512u + ((uint32_t)gz & 7u) * 64u + obit, &d.hdr->retries);
            }
          }
        }
      });
    }
  }
}

__global__ __launch_bounds__(256) void isl_flatten(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    uint64_t M[8];
    uint32_t n = 0;
    if (isl_load_brick(s.seg, b, M)) {
#pragma unroll
      for (int z = 0; z < 8; ++z) {
        bool root = false;
        if ((M[z] >> lane) & 1ull) {
          const uint32_t me = b * 512u + (uint32_t)z * 64u + lane;
          uint32_t r = d.lab[me], q;
          while ((q = d.lab[r]) != r) r = q;
          d.lab[me] = r;
          root = r == me;
        }
        n += (uint32_t)__popcll(__ballot(root));
      }
    }
    if (lane == 0u) d.nroots[b] = n;
  }
}

// one workgroup of 1024: thread t owns the bricks [t * chunk, (t + 1) * chunk)
__global__ __launch_bounds__(1024) void isl_scan(const SegDev s, const IslDev d) {
  __shared__ uint32_t part[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (s.nb + 1023u) / 1024u;
  const uint32_t b0 = min(s.nb, t * chunk), b1 = min(s.nb, b0 + chunk);
  uint32_t a = 0;
  for (uint32_t b = b0; b < b1; ++b) a += d.nroots[b];
  part[t] = a;
  __syncthreads();
  if (t == 0u) {
    uint32_t run = 0;
    for (uint32_t k = 0; k < 1024u; ++k) {
      const uint32_t v = part[k];
      part[k] = run;
      run += v;
    }
    d.hdr->roots = run;
  }
  __syncthreads();
  a = part[t];
  for (uint32_t b = b0; b < b1; ++b) {
    d.off[b] = a;
    a += d.nroots[b];
  }
}

__global__ __launch_bounds__(256) void isl_rootid(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    if (d.nroots[b] == 0u) continue;
    uint64_t M[8];
    isl_load_brick(s.seg, b, M);
    uint32_t base = d.off[b];
#pragma unroll
    for (int z = 0; z < 8; ++z) {
      const uint32_t me = b * 512u + (uint32_t)z * 64u + lane;
      const bool root = ((M[z] >> lane) & 1ull) && d.lab[me] == me;
      const uint64_t bal = __ballot(root);
      if (root) {
        const uint32_t row = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (row < d.cap) {   // (the host sized the table with isl_scan's total)
          d.lab[me] = ISL_ID | row;
          IslRow r;
          r.count = 0;
          r.anchor = 0xffffffffu;
          for (int a = 0; a < 3; ++a) {
            r.lo[a] = 0xffffffffu;
            r.hi[a] = 0u;
          }
          r.pad = 0u;
          d.rows[row] = r;
        }
      }
      base += (uint32_t)__popcll(bal);
    }
  }
}

// a min / max that skips the read-modify-write when the word already is at least as good: the words only move one way, so a
// value read earlier can only be worse than the present one
VXD void isl_min(uint32_t* p, uint32_t v) {
  if (__hip_atomic_load(p, ISL_RLX_AGENT) > v) atomicMin(p, v);
}
VXD void isl_max(uint32_t* p, uint32_t v) {
  if (__hip_atomic_load(p, ISL_RLX_AGENT) < v) atomicMax(p, v);
}

// a run of voxels of one row inside a brick, in (z, y, x) order: wave uniform
struct IslRun {
  uint32_t row, count, anchor;
  uint32_t cols, rows, zl, zh;
};

VXD void isl_flush(const IslDev& d, const IslRun& a, uint32_t bx, uint32_t by, uint32_t bz, uint32_t lane) {
  if (a.row == ISL_NONE || a.row >= d.cap || lane != 0u) return;
  IslRow* r = d.rows + a.row;
  atomicAdd(&r->count, (unsigned long long)a.count);
  isl_min(&r->anchor, a.anchor);
  isl_min(&r->lo[0], bx * 8u + (uint32_t)(__ffs(a.cols) - 1));
  isl_max(&r->hi[0], bx * 8u + (uint32_t)(31 - __clz(a.cols)));
  isl_min(&r->lo[1], by * 8u + (uint32_t)(__ffs(a.rows) - 1));
  isl_max(&r->hi[1], by * 8u + (uint32_t)(31 - __clz(a.rows)));
  isl_min(&r->lo[2], bz * 8u + a.zl);
  isl_max(&r->hi[2], bz * 8u + a.zh);
}

__global__ __launch_bounds__(256) void isl_table(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * 4u;
  const uint32_t X = s.bc[0] * 8u, Y = s.bc[1] * 8u;
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    uint64_t M[8];
    if (!isl_load_brick(s.seg, b, M)) continue;
    const uint32_t bx = b % s.bc[0], t = b / s.bc[0], by = t % s.bc[1], bz = t / s.bc[1];
    IslRun run{ISL_NONE, 0u, 0u, 0u, 0u, 0u, 0u};
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      const bool set = (M[z] >> lane) & 1ull;
      uint32_t row = ISL_NONE;
      if (set) {
        const uint32_t me = b * 512u + z * 64u + lane;
        uint32_t l = d.lab[me];
        // isl_flatten left the root here and isl_rootid gave every root its row: one step.  The bound only keeps a table
        // that was sized too small from turning into an endless walk (such a voxel joins no row).
        for (uint32_t hop = 0; hop < 64u && !(l & ISL_ID); ++hop) l = d.lab[l];
        if (l & ISL_ID) {
          d.lab[me] = l;
          row = l & ~ISL_ID;
        }
      }
      uint64_t rem = M[z];
      while (rem) {
        const uint32_t first = (uint32_t)__ffsll((unsigned long long)rem) - 1u;
        const uint32_t cur = (uint32_t)__shfl((int)row, (int)first);
        const uint64_t m = __ballot(set && row == cur);
        rem &= ~m;
        if (cur != run.row) {
          isl_flush(d, run, bx, by, bz, lane);
          run = IslRun{cur, 0u, ((bz * 8u + z) * Y + by * 8u + (first >> 3)) * X + bx * 8u + (first & 7u), 0u, 0u, z, z};
        }
        run.count += (uint32_t)__popcll(m);
#pragma unroll
        for (int r = 0; r < 8; ++r) {
          const uint32_t rw = (uint32_t)(m >> (8 * r)) & 255u;
          run.cols |= rw;
          run.rows |= rw ? 1u << r : 0u;
        }
        run.zh = z;
      }
    }
    isl_flush(d, run, bx, by, bz, lane);
  }
}

// one lane: the row of voxel (b, z, bit), ISL_NONE when the voxel is not set (after isl_table: every set voxel holds its row)
__global__ void isl_seed_row(const SegDev s, const IslDev d, const SegSeed seed) {
  if (threadIdx.x != 0u || blockIdx.x != 0u) return;
  const bool on = (s.seg[(size_t)seed.b * 8u + seed.z] & seed.bit) != 0;
  const uint32_t bit = (uint32_t)__ffsll((unsigned long long)seed.bit) - 1u;
  d.hdr->seed_row = on ? d.lab[(size_t)seed.b * 512u + seed.z * 64u + bit] & ~ISL_ID : ISL_NONE;
}

// the mask after an op: a voxel stays when its row keeps a label.  Each wave reads and writes its own brick only.
__global__ __launch_bounds__(256) void isl_apply(const SegDev s, const IslDev d) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t b = isl_wave_brick(); b < s.nb; b += waves) {
    uint64_t M[8];
    if (!isl_load_brick(s.seg, b, M)) continue;
    uint64_t mine = 0;
#pragma unroll
    for (uint32_t z = 0; z < 8u; ++z) {
      bool keep = false;
      if ((M[z] >> lane) & 1ull) {
        const uint32_t row = d.lab[(size_t)b * 512u + z * 64u + lane] & ~ISL_ID;
        keep = row < d.cap && d.newlab[row] != 0u;
      }
      const uint64_t w = __ballot(keep);
      mine = lane == z ? w : mine;
    }
    if (lane < 8u) s.seg[(size_t)b * 8u + lane] = mine;
  }
}

// the dense label volume: out[(z * Y + y) * X + x] = the label of voxel (x, y, z), 0 outside the mask
__global__ __launch_bounds__(256) void isl_labels_out(const SegDev s, const IslDev d, uint32_t X, uint32_t Y, size_t nvox,
                                                      uint32_t* __restrict__ out) {
  const size_t stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < nvox; k += stride) {
    const uint32_t x = (uint32_t)(k % X);
    const size_t r = k / X;
    const uint32_t y = (uint32_t)(r % Y), z = (uint32_t)(r / Y);
    const uint32_t b = ((z >> 3) * s.bc[1] + (y >> 3)) * s.bc[0] + (x >> 3);
    const uint32_t bit = ((y & 7u) << 3) | (x & 7u);
    uint32_t l = 0u;
    if ((s.seg[(size_t)b * 8u + (z & 7u)] >> bit) & 1ull) {
      const uint32_t row = d.lab[(size_t)b * 512u + (z & 7u) * 64u + bit] & ~ISL_ID;
      l = row < d.cap ? d.newlab[row] : 0u;
    }
    out[k] = l;
  }
}

}  // namespace vx
