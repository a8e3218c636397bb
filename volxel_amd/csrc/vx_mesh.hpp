// vx_mesh.hpp -- surface meshes of isosurfaces and segments (vx_mesh_extract, DESIGN.md section 2 "Meshes"): naive surface nets,
// one vertex per grid cell the surface passes through, one quad (two triangles) per grid edge it crosses.
//
// "Inside" is kept as the brick-major bit words of vx_segment.hpp (brick b: 8 x u64, word z, bit y * 8 + x), in a buffer the
// mesher owns.  Cells are grouped in cell blocks: block B (B_a in [0, bricks_a], x fastest) holds the cells 8B - 1 .. 8B + 6 per
// axis, whose corners are the voxels 8B - 1 .. 8B + 7: the bricks B - {0, 1}^3, an absent brick reading 0.
//   mesh_inside_density<LAYOUT>  one wave per brick, one ballot per z slice: d(i) >= iso inside the box.  A brick whose range
//                                (the f16 pair, widened) lies wholly below iso writes zeros, wholly at or above it the box
//                                pattern, neither reading a voxel.
//   mesh_inside_segment          the segment's words AND the box pattern.
//   mesh_active                  one lane per cell block: the active-cell words (the eight corner planes by shifts of the
//                                inside words: active = not all equal), the block's vertex and quad counts by popcounts, the
//                                cell bbox and the number of active blocks (integer atomics: order-free results), and the
//                                workgroup's sums of both counts.
//   mesh_scan_partials / mesh_offsets   the exclusive scan of the counts: the workgroup sums scanned by one workgroup, then
//                                each workgroup's local scan on top of its offset.  Plain launches in stream order.
//   mesh_emit<LAYOUT, SEGMENT>   one wave per active block, lane = (y, x), a loop over z: the block's 9^3 corner values staged
//                                in LDS, the vertex of every active cell and the two triangles of every crossing edge the block
//                                owns (the edge from voxel p along an axis belongs to cell p).  A vertex's index is its block's
//                                offset plus the popcount of the block's active bits below its own; a quad's slot is the
//                                block's quad offset plus the crossings before it in (z, axis, bit) order: functions of the
//                                input only.  No slot is claimed with an atomic.
// The discipline of vx_segment.hpp holds: no spin, no decoupled look-back, no grid barrier, no cooperative or persistent launch;
// every output word has one writer, and every write is guarded by the totals the host sized the outputs with.
#pragma once

#include "vx_device.hpp"

namespace vx {

struct MeshBox {
  uint32_t lo[3], hi[3];
};

// word z of brick (bx, by, bz), 0 for a brick outside the grid
VXD uint64_t mesh_word(const uint64_t* __restrict__ w, const uint32_t (&bc)[3], int bx, int by, int bz, uint32_t z) {
  const bool ok = (uint32_t)bx < bc[0] && (uint32_t)by < bc[1] && (uint32_t)bz < bc[2];
  return ok ? w[((size_t)((uint32_t)bz * bc[1] + (uint32_t)by) * bc[0] + (uint32_t)bx) * 8u + z] : 0ull;
}

// the voxels of the box in slice z of brick (bx, by, bz), as a word
VXD uint64_t mesh_box_word(const MeshBox& box, uint32_t bx, uint32_t by, uint32_t bz, uint32_t z) {
  const uint32_t zz = bz * 8u + z;
  if (zz < box.lo[2] || zz > box.hi[2]) return 0ull;
  uint32_t mx = 0, my = 0;
#pragma unroll
  for (uint32_t k = 0; k < 8u; ++k) {
    const uint32_t x = bx * 8u + k, y = by * 8u + k;
    mx |= (x >= box.lo[0] && x <= box.hi[0]) ? 1u << k : 0u;
    my |= (y >= box.lo[1] && y <= box.hi[1]) ? 1u << k : 0u;
  }
  uint64_t w = 0;
#pragma unroll
  for (uint32_t y = 0; y < 8u; ++y) w |= ((my >> y) & 1u) ? (uint64_t)mx << (8u * y) : 0ull;
  return w;
}

VXD void mesh_reset(const MeshDev& m) {
  if (blockIdx.x == 0u && threadIdx.x == 0u) {
    MeshStats* st = m.st;
    st->verts = 0;
    st->quads = 0;
    st->active_blocks = 0;
    for (int a = 0; a < 3; ++a) {
      st->lo[a] = 0xffffffffu;
      st->hi[a] = 0u;
    }
  }
}

// A decoded voxel of brick b, fma(code / 255, max - min, min), lies within a few roundings (2^-22 of the larger magnitude) of
// [min, max]; the two products by scale and inv_maj are monotone for positive factors.  The range widened by 2^-16 of the
// magnitude therefore bounds every d of the brick; other factors, or a NaN anywhere, decide nothing (every comparison is false).
template <int LAYOUT>
__global__ __launch_bounds__(256) void mesh_inside_density(const DevVolume v, float scale, float inv_maj, float iso, const MeshBox box,
                                                           const MeshDev m) {
  mesh_reset(m);
  const uint32_t lane = threadIdx.x & 63u, lx = lane & 7u, ly = lane >> 3;
  const uint32_t waves = gridDim.x * 4u;
  const bool monotone = scale > 0.0f && inv_maj > 0.0f && scale < __int_as_float(0x7f800000) && inv_maj < __int_as_float(0x7f800000);
  for (uint32_t b = blockIdx.x * 4u + (threadIdx.x >> 6); b < m.nb; b += waves) {   // wave uniform
    const uint32_t bx = b % m.bc[0], t = b / m.bc[0], by = t % m.bc[1], bz = t / m.bc[1];
    const uint32_t rg = v.range[b];
    const float ra = half_bits_to_float(rg >> 16), rb = half_bits_to_float(rg & 0xffffu);
    const float mn = fminf(ra, rb), mx = fmaxf(ra, rb), mag = fmaxf(fabsf(mn), fabsf(mx)) * 0x1p-16f;
    const float dlo = (scale * (mn - mag)) * inv_maj, dhi = (scale * (mx + mag)) * inv_maj;
    const bool below = monotone && dhi < iso, above = monotone && dlo >= iso;
    uint64_t mine = 0;
    if (below || above) {   // wave uniform
      if (lane < 8u) mine = above ? mesh_box_word(box, bx, by, bz, lane) : 0ull;
    } else {
      const uint32_t x = bx * 8u + lx, y = by * 8u + ly;
      const bool in_xy = x >= box.lo[0] && x <= box.hi[0] && y >= box.lo[1] && y <= box.hi[1];
#pragma unroll
      for (uint32_t z = 0; z < 8u; ++z) {
        const uint32_t zz = bz * 8u + z;
        const float d = seg_density<LAYOUT>(v, scale, inv_maj, x, y, zz);
        const uint64_t w = __ballot(in_xy && zz >= box.lo[2] && zz <= box.hi[2] && d >= iso);
        mine = lane == z ? w : mine;
      }
    }
    if (lane < 8u) m.inside[(size_t)b * 8u + lane] = mine;
  }
}

// one lane per word
__global__ __launch_bounds__(256) void mesh_inside_segment(const uint64_t* __restrict__ seg, const MeshBox box, const MeshDev m) {
  mesh_reset(m);
  const size_t n = (size_t)m.nb * 8u, stride = (size_t)gridDim.x * blockDim.x;
  for (size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x; k < n; k += stride) {
    const uint32_t b = (uint32_t)(k >> 3), z = (uint32_t)(k & 7u);
    const uint32_t bx = b % m.bc[0], t = b / m.bc[0], by = t % m.bc[1], bz = t / m.bc[1];
    m.inside[k] = seg[k] & mesh_box_word(box, bx, by, bz, z);
  }
}

// The four corner planes (ox, oy) of one z slab of cell block (Bx, By): bit (y, x) of plane (ox, oy) is voxel
// (8Bx - 1 + x + ox, 8By - 1 + y + oy) of the slab.  w[dy][dx] is the slab's word of brick (Bx - dx, By - dy).
struct MeshPlanes {
  uint64_t p[2][2];   // [ox][oy]
};
VXD MeshPlanes mesh_planes(uint64_t w00, uint64_t w01, uint64_t w10, uint64_t w11) {   // w<dy><dx>
  const uint64_t y1 = (w00 << 8) | (w10 >> 56);   // bricks Bx: rows moved up by one, row 0 from the brick below in y
  const uint64_t y0 = (w01 << 8) | (w11 >> 56);   // bricks Bx - 1
  MeshPlanes r;
  r.p[1][1] = w00;
  r.p[0][1] = ((w00 & ~SEG_COL7) << 1) | ((w01 & SEG_COL7) >> 7);
  r.p[1][0] = y1;
  r.p[0][0] = ((y1 & ~SEG_COL7) << 1) | ((y0 & SEG_COL7) >> 7);
  return r;
}

// one lane per cell block; grid = np workgroups of 256
__global__ __launch_bounds__(256) void mesh_active(const MeshDev m) {
  __shared__ uint32_t red[2][4];
  const uint32_t B = blockIdx.x * 256u + threadIdx.x;
  uint32_t nv = 0, nq = 0;
  if (B < m.ncb) {
    const int Bx = (int)(B % m.cb[0]), By = (int)((B / m.cb[0]) % m.cb[1]), Bz = (int)(B / (m.cb[0] * m.cb[1]));
    MeshPlanes prev{};
    uint64_t A[8], u = 0;
    uint32_t zl = 8, zh = 0;
#pragma unroll
    for (int vz = 0; vz < 9; ++vz) {
      const int bz = vz == 0 ? Bz - 1 : Bz;
      const uint32_t z = vz == 0 ? 7u : (uint32_t)(vz - 1);
      const MeshPlanes cur = mesh_planes(mesh_word(m.inside, m.bc, Bx, By, bz, z), mesh_word(m.inside, m.bc, Bx - 1, By, bz, z),
                                         mesh_word(m.inside, m.bc, Bx, By - 1, bz, z), mesh_word(m.inside, m.bc, Bx - 1, By - 1, bz, z));
      if (vz > 0) {
        const uint64_t any = prev.p[0][0] | prev.p[0][1] | prev.p[1][0] | prev.p[1][1] | cur.p[0][0] | cur.p[0][1] | cur.p[1][0] | cur.p[1][1];
        const uint64_t all = prev.p[0][0] & prev.p[0][1] & prev.p[1][0] & prev.p[1][1] & cur.p[0][0] & cur.p[0][1] & cur.p[1][0] & cur.p[1][1];
        const uint64_t a = any & ~all;
        A[vz - 1] = a;
        nv += (uint32_t)__popcll(a);
        nq += (uint32_t)(__popcll(prev.p[0][0] ^ prev.p[1][0]) + __popcll(prev.p[0][0] ^ prev.p[0][1]) + __popcll(prev.p[0][0] ^ cur.p[0][0]));
        u |= a;
        if (a) {
          zl = min(zl, (uint32_t)(vz - 1));
          zh = (uint32_t)(vz - 1);
        }
      }
      prev = cur;
    }
    ulonglong2* ao = reinterpret_cast<ulonglong2*>(m.act + (size_t)B * 8u);
#pragma unroll
    for (int k = 0; k < 4; ++k) ao[k] = make_ulonglong2(A[2 * k], A[2 * k + 1]);
    m.vq[B] = make_uint2(nv, nq);
    if (nv) {
      uint32_t cols = 0, rows = 0;
#pragma unroll
      for (int r = 0; r < 8; ++r) {
        const uint32_t row = (uint32_t)(u >> (8 * r)) & 255u;
        cols |= row;
        rows |= row ? 1u << r : 0u;
      }
      MeshStats* st = m.st;
      atomicAdd(&st->active_blocks, 1ull);
      atomicMin(&st->lo[0], (uint32_t)Bx * 8u + (uint32_t)(__ffs(cols) - 1));
      atomicMax(&st->hi[0], (uint32_t)Bx * 8u + (uint32_t)(31 - __clz(cols)));
      atomicMin(&st->lo[1], (uint32_t)By * 8u + (uint32_t)(__ffs(rows) - 1));
      atomicMax(&st->hi[1], (uint32_t)By * 8u + (uint32_t)(31 - __clz(rows)));
      atomicMin(&st->lo[2], (uint32_t)Bz * 8u + zl);
      atomicMax(&st->hi[2], (uint32_t)Bz * 8u + zh);
    }
  }
  uint32_t sv = nv, sq = nq;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    sv += __shfl_xor(sv, o);
    sq += __shfl_xor(sq, o);
  }
  if ((threadIdx.x & 63u) == 0u) {
    red[0][threadIdx.x >> 6] = sv;
    red[1][threadIdx.x >> 6] = sq;
  }
  __syncthreads();
  if (threadIdx.x == 0u) m.part[blockIdx.x] = make_uint2(red[0][0] + red[0][1] + red[0][2] + red[0][3], red[1][0] + red[1][1] + red[1][2] + red[1][3]);
}

// one workgroup of 1024: thread t owns the workgroup sums [t * chunk, (t + 1) * chunk); the totals go to the statistics in
// 64 bits (the host refuses a mesh beyond 32-bit indices before anything is emitted), the offsets wrap in 32
__global__ __launch_bounds__(1024) void mesh_scan_partials(const MeshDev m) {
  __shared__ unsigned long long sv[1024], sq[1024];
  const uint32_t t = threadIdx.x;
  const uint32_t chunk = (m.np + 1023u) / 1024u;
  const uint32_t i0 = min(m.np, t * chunk), i1 = min(m.np, i0 + chunk);
  unsigned long long v = 0, q = 0;
  for (uint32_t i = i0; i < i1; ++i) {
    const uint2 p = m.part[i];
    v += p.x;
    q += p.y;
  }
  sv[t] = v;
  sq[t] = q;
  __syncthreads();
  if (t == 0u) {
    unsigned long long rv = 0, rq = 0;
    for (uint32_t k = 0; k < 1024u; ++k) {
      const unsigned long long a = sv[k], b = sq[k];
      sv[k] = rv;
      sq[k] = rq;
      rv += a;
      rq += b;
    }
    m.st->verts = rv;
    m.st->quads = rq;
  }
  __syncthreads();
  v = sv[t];
  q = sq[t];
  for (uint32_t i = i0; i < i1; ++i) {
    const uint2 p = m.part[i];
    m.poff[i] = make_uint2((uint32_t)v, (uint32_t)q);
    v += p.x;
    q += p.y;
  }
}

// grid = np workgroups of 256, the blocks of mesh_active's workgroups
__global__ __launch_bounds__(256) void mesh_offsets(const MeshDev m) {
  __shared__ uint32_t tot[2][4];
  const uint32_t B = blockIdx.x * 256u + threadIdx.x, lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  const uint2 c = B < m.ncb ? m.vq[B] : make_uint2(0u, 0u);
  uint32_t iv = c.x, iq = c.y;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t a = __shfl_up(iv, o), b = __shfl_up(iq, o);
    iv += lane >= (uint32_t)o ? a : 0u;
    iq += lane >= (uint32_t)o ? b : 0u;
  }
  if (lane == 63u) {
    tot[0][wave] = iv;
    tot[1][wave] = iq;
  }
  __syncthreads();
  const uint2 base = m.poff[blockIdx.x];
  uint32_t bv = base.x, bq = base.y;
  for (uint32_t w = 0; w < wave; ++w) {
    bv += tot[0][w];
    bq += tot[1][w];
  }
  if (B < m.ncb) m.off[B] = make_uint2(bv + iv - c.x, bq + iq - c.y);
}

// the per-wave LDS of mesh_emit: the 9^3 corner values and the rank tables of the eight blocks B - {0, 1}^3
struct MeshLds {
  float f[9 * 9 * 9 + 3];
  uint32_t pre[8][8];    // slot k = dx | dy << 1 | dz << 2: the block's vertex offset + the active cells of its words below z
  uint64_t aw[8][8];     // its active words
};

// the index of the vertex of the cell at (x, y, z) in [-1, 7]^3 of this block's frame
VXD uint32_t mesh_index(const MeshLds& s, int x, int y, int z) {
  const uint32_t k = (x < 0 ? 1u : 0u) | (y < 0 ? 2u : 0u) | (z < 0 ? 4u : 0u);
  const uint32_t lz = (uint32_t)z & 7u, bit = (((uint32_t)y & 7u) << 3) | ((uint32_t)x & 7u);
  return s.pre[k][lz] + (uint32_t)__popcll(s.aw[k][lz] & ((1ull << bit) - 1ull));
}

VXD void mesh_store_quad(uint32_t* __restrict__ tris, size_t q, bool fwd, uint32_t k0, uint32_t k1, uint32_t k2, uint32_t k3) {
  uint2* o = reinterpret_cast<uint2*>(tris + q * 6u);   // 24 bytes per quad: 8-byte aligned
  const uint32_t b = fwd ? k1 : k3, d = fwd ? k3 : k1;
  o[0] = make_uint2(k0, b);
  o[1] = make_uint2(k2, k0);
  o[2] = make_uint2(k2, d);
}

// one crossing edge of a cell: f0 at the lower corner (ox, oy, oz), f1 one step along AXIS
template <int AXIS>
VXD void mesh_edge(float f0, float f1, float iso, float ox, float oy, float oz, float& sx, float& sy, float& sz, uint32_t& n) {
  if ((f0 >= iso) != (f1 >= iso)) {
    const float t = fminf(fmaxf((iso - f0) / (f1 - f0), 0.0f), 1.0f);
    sx += AXIS == 0 ? t : ox;
    sy += AXIS == 1 ? t : oy;
    sz += AXIS == 2 ? t : oz;
    n += 1u;
  }
}

template <int LAYOUT, bool SEGMENT>
__global__ __launch_bounds__(256) void mesh_emit(const DevVolume v, float scale, float inv_maj, float iso, const MeshBox box, const MeshDev m,
                                                 unsigned long long nverts, unsigned long long nquads, float* __restrict__ verts,
                                                 int32_t* __restrict__ cells, uint32_t* __restrict__ tris) {
  __shared__ MeshLds lds[4];
  MeshLds& s = lds[threadIdx.x >> 6];
  const uint32_t lane = threadIdx.x & 63u;
  const int lx = (int)(lane & 7u), ly = (int)(lane >> 3);
  const uint32_t waves = gridDim.x * 4u;
  for (uint32_t B = blockIdx.x * 4u + (threadIdx.x >> 6); B < m.ncb; B += waves) {   // wave uniform
    if (m.vq[B].x == 0u) continue;
    const int Bx = (int)(B % m.cb[0]), By = (int)((B / m.cb[0]) % m.cb[1]), Bz = (int)(B / (m.cb[0] * m.cb[1]));
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");   // the last block's reads of this LDS are done
    __builtin_amdgcn_wave_barrier();
    {   // rank tables: lane = slot * 8 + z
      const uint32_t k = lane >> 3, z = lane & 7u;
      const int nx = Bx - (int)(k & 1u), ny = By - (int)((k >> 1) & 1u), nz = Bz - (int)(k >> 2);
      const bool ok = nx >= 0 && ny >= 0 && nz >= 0;
      const uint32_t nb = ok ? ((uint32_t)nz * m.cb[1] + (uint32_t)ny) * m.cb[0] + (uint32_t)nx : 0u;
      const uint64_t w = ok ? m.act[(size_t)nb * 8u + z] : 0ull;
      s.aw[k][z] = w;
      uint32_t incl = (uint32_t)__popcll(w);   // inclusive scan over the slot's 8 lanes
      const uint32_t own = incl;
#pragma unroll
      for (int o = 1; o < 8; o <<= 1) {
        const uint32_t a = __shfl_up(incl, o);
        incl += z >= (uint32_t)o ? a : 0u;
      }
      s.pre[k][z] = (ok ? m.off[nb].x : 0u) + incl - own;
    }
    // the corner values: voxel (8B - 1 + vx, ...) at f[(vz * 9 + vy) * 9 + vx]; outside the box or the volume: 0
    for (uint32_t i = lane; i < 729u; i += 64u) {
      const uint32_t vx = i % 9u, vy = (i / 9u) % 9u, vz = i / 81u;
      const int x = Bx * 8 - 1 + (int)vx, y = By * 8 - 1 + (int)vy, z = Bz * 8 - 1 + (int)vz;
      float f;
      if (SEGMENT) {
        const uint64_t w = mesh_word(m.inside, m.bc, x >> 3, y >> 3, z >> 3, (uint32_t)z & 7u);
        f = (w >> ((((uint32_t)y & 7u) << 3) | ((uint32_t)x & 7u))) & 1ull ? 1.0f : 0.0f;
      } else {
        const bool in = (uint32_t)x >= box.lo[0] && (uint32_t)x <= box.hi[0] && (uint32_t)y >= box.lo[1] && (uint32_t)y <= box.hi[1] &&
                        (uint32_t)z >= box.lo[2] && (uint32_t)z <= box.hi[2] && x >= 0 && y >= 0 && z >= 0;
        const float d = (scale * lookup_density_nearest<LAYOUT>(v, x, y, z)) * inv_maj;
        f = in ? d : 0.0f;
      }
      s.f[i] = f;
    }
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const uint2 off = m.off[B];
    uint32_t qbase = off.y;
    for (int lz = 0; lz < 8; ++lz) {
      const uint64_t A = s.aw[0][lz];
      if (!A) continue;   // wave uniform: no active cell, so no crossing edge either
      float c[2][2][2];   // [oz][oy][ox]
#pragma unroll
      for (int oz = 0; oz < 2; ++oz)
#pragma unroll
        for (int oy = 0; oy < 2; ++oy)
#pragma unroll
          for (int ox = 0; ox < 2; ++ox) c[oz][oy][ox] = s.f[((lz + oz) * 9 + ly + oy) * 9 + lx + ox];
      if ((A >> lane) & 1ull) {
        float sx = 0.0f, sy = 0.0f, sz = 0.0f;
        uint32_t n = 0;
        // the contract's order: x-edges by (z, y), y-edges by (z, x), z-edges by (y, x)
#pragma unroll
        for (int e = 0; e < 4; ++e) mesh_edge<0>(c[e >> 1][e & 1][0], c[e >> 1][e & 1][1], iso, 0.0f, (float)(e & 1), (float)(e >> 1), sx, sy, sz, n);
#pragma unroll
        for (int e = 0; e < 4; ++e) mesh_edge<1>(c[e >> 1][0][e & 1], c[e >> 1][1][e & 1], iso, (float)(e & 1), 0.0f, (float)(e >> 1), sx, sy, sz, n);
#pragma unroll
        for (int e = 0; e < 4; ++e) mesh_edge<2>(c[0][e >> 1][e & 1], c[1][e >> 1][e & 1], iso, (float)(e & 1), (float)(e >> 1), 0.0f, sx, sy, sz, n);
        const float fn = (float)n;
        const int cx = Bx * 8 - 1 + lx, cy = By * 8 - 1 + ly, cz = Bz * 8 - 1 + lz;
        const size_t at = (size_t)mesh_index(s, lx, ly, lz);
        if (n != 0u && at < nverts) {
          verts[at * 3u] = (float)cx + sx / fn;
          verts[at * 3u + 1u] = (float)cy + sy / fn;
          verts[at * 3u + 2u] = (float)cz + sz / fn;
          cells[at * 3u] = cx;
          cells[at * 3u + 1u] = cy;
          cells[at * 3u + 2u] = cz;
        }
      }
      // the edges this cell owns: from its corner (0, 0, 0) along x, y and z
      const bool in0 = c[0][0][0] >= iso;
      const bool ex = in0 != (c[0][0][1] >= iso), ey = in0 != (c[0][1][0] >= iso), ez = in0 != (c[1][0][0] >= iso);
      const uint64_t wx = __ballot(ex), wy = __ballot(ey), wz = __ballot(ez);
      const uint64_t below = (1ull << lane) - 1ull;
      const uint32_t qx = qbase + (uint32_t)__popcll(wx & below);
      const uint32_t qy = qbase + (uint32_t)__popcll(wx) + (uint32_t)__popcll(wy & below);
      const uint32_t qz = qbase + (uint32_t)__popcll(wx) + (uint32_t)__popcll(wy) + (uint32_t)__popcll(wz & below);
      qbase += (uint32_t)(__popcll(wx) + __popcll(wy) + __popcll(wz));
      const uint32_t k11 = (ex || ey || ez) ? mesh_index(s, lx, ly, lz) : 0u;
      // the quad c00, c10 = c00 + e_u, c11 = the cell, c01 = c00 + e_v, with (u, v) the cyclic partners of the axis
      if (ex && qx < nquads)
        mesh_store_quad(tris, qx, in0, mesh_index(s, lx, ly - 1, lz - 1), mesh_index(s, lx, ly, lz - 1), k11, mesh_index(s, lx, ly - 1, lz));
      if (ey && qy < nquads)
        mesh_store_quad(tris, qy, in0, mesh_index(s, lx - 1, ly, lz - 1), mesh_index(s, lx - 1, ly, lz), k11, mesh_index(s, lx, ly, lz - 1));
      if (ez && qz < nquads)
        mesh_store_quad(tris, qz, in0, mesh_index(s, lx - 1, ly - 1, lz), mesh_index(s, lx, ly - 1, lz), k11, mesh_index(s, lx - 1, ly, lz));
    }
  }
}

}  // namespace vx
