// vx_types.hpp -- the plain structs that cross the host / device line and that VxContext (vx_context.hpp) holds by value: the
// device view of the volume, the tile map, the per-wave counter record, and the device-side descriptions of the light grid,
// the isosurface bounds, the segment, the islands and the mesh, each with the structs it points to.  No function, no kernel:
// the host units include it without a kernel header, the kernel headers through vx_device.hpp.  A struct that is only ever a
// kernel argument of one feature (SegSeed, SegPredParams, MeshBox, LightMarch, MultiOut, MergeArgs) stays beside its kernels.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/volxel_hip.h"

namespace vx {

// ---------------------------------------------------------------------------------------
// device view of an uploaded volume
struct DevVolume {
  // reference layout: the three textures of viewer.ts:1106-1142 as linear buffers
  const uint32_t* indirection;  // 10-10-10 pointers            (brick.rs:30-35)
  const uint32_t* range;        // (f16 min << 16) | f16 max    (brick.rs:19-23)
  const uint8_t* atlas;         // u8 voxels, x fastest         (buf3d.rs:26-28)
  const uint32_t* mips[3];      // range mips, GL levels 1..3   (brick.rs:153-190)
  uint32_t bc[3];               // bricks per axis (= indirection = range dims)
  uint32_t atlas_size[3];
  uint32_t extent[3];           // padded index extent = bc*8   (brick.rs:236-238)
  uint32_t mip_size[3][3];
  // MI355X layout "cellquad": apron bricks of pre-decoded fp32 xy-quads
  const float4* cq;             // [(bc+1)^3][9 slices][8][8] float4
  uint32_t cq_bc[3];            // bc + 1
  // MI355X layout "brickf32": every 8^3 brick decoded to fp32, 2 KiB contiguous, brick-major
  const float* bf;              // [bc.z][bc.y][bc.x][8][8][8], one all-zero 16-byte chunk behind the last brick
  uint32_t bf_zero;             // index (in floats) of that chunk, or 0 when the layout needs more than 32 index bits
  // MI355X layout "bricku8" (opt-in): the same bricks as the atlas' 8-bit codes, 4 per dword, dword index = the
  // 16-byte-unit index of brickf32 (brick * 128 + z * 16 + y * 2 + (x >> 2)); one zero dword behind the last brick.
  // bu_range[b] = {min, max - min} of brick b (range texture, decoded from f16); the entry behind the last brick is
  // {0, 0}: it serves the zero dword, so rows and chunks outside the volume decode to 0 (A4).
  const uint32_t* bu;
  const float2* bu_range;
  uint32_t bu_active;           // unused: vx_api.hip plan_launch decides U8; kept so the offsets behind it stay
  // exact empty-space skipping (DVR): one bit per macro cell of 8 << skip_level voxels
  const uint32_t* skip_bits;    // nullptr: none
  uint32_t skip_level;
  uint32_t skip_dims[3];        // (extent >> (3 + level)) + 1
  uint32_t skip_words;
  // default mode (A13): the local majorant maj * TF(scale * range max).a of every cell of range-texture levels 0..3
  // (dda.glsl:36,78), levels back to back, each at the strides of level 0; entry lmaj_cells = the value outside
  const float* lmaj;            // built by vx_api before a `default` launch (build_local_majorants)
  uint32_t lmaj_cells;          // 4 * bricks
  // environment map (environment.ts): RGBA32F texels in GL row order + importance mip pyramid
  const float4* env_tex;        // nullptr: none (directional light only)
  uint32_t env_w, env_h;
  const float* env_imp;         // levels 0..9 of the 512^2 map back to back (imp_offset)
  const float4* env_impq;       // the same levels 0..8 as 2x2 sibling quads, one 16-byte load per level
  float env_avg_w;              // level 9 (the mean importance)
  // wave-uniform terms of the primary ray, evaluated once per launch on the host with the device's own operations
  // (IEEE fma chains and divisions: vx_api.hip derive_camera) instead of once per wave on the vector ALUs -- the
  // reference hoists its matrix inverses the same way (quirk Q11).  Perspective camera only (an orthographic ray's
  // origin is per pixel); read by the tuned DVR kernels through dvr_setup.
  float cam_o[3];               // inverse(view) * (0,0,0,1), divided by w          (utils.glsl:25-27)
  float cam_ipos[3];            // density_transform_inv * (cam_o, 1)               (to_index of the origin)
  float inv_res[2];             // 1 / u_res
  // Round 4: two more per-ray divisions decided per launch on the host (vx_api.hip prepare_render), both exact:
  //  * RAY_AFFINE_VIEW: inverse(view) has the bottom row (0,0,0,1), so the w of inverse(view) * (v, 1) is fma(1, 1, 0 * ...)
  //    = 1.0 and the three divisions by it (utils.glsl:35-37) return their numerators;
  //  * RAY_TEX_BY_RECIPROCAL: (pixel + 0.5) / res over the whole image equals the quotient corrected once with the rounded
  //    reciprocal -- q0 = a * y, q = fma(fma(-res, q0, a), y, q0) -- for EVERY pixel coordinate of this resolution (the host
  //    tries all of them against the IEEE division; a resolution for which one differs keeps the division).
  uint32_t ray_flags;
};
constexpr uint32_t RAY_AFFINE_VIEW = 1u, RAY_TEX_BY_RECIPROCAL_X = 2u, RAY_TEX_BY_RECIPROCAL_Y = 4u;

// the device layout a kernel instance samples (its LAYOUT template argument)
enum { LAYOUT_REF = 0, LAYOUT_CQ = 1, LAYOUT_BF = 2 };

// image <-> slab mapping: 64x64-pixel sharding tiles dealt
// round-robin to shards; inside a tile 64 wave-tiles of 8x8 pixels in Morton order; the
// accumulator ("slab") is tile-major so that one wave owns 1 KiB of contiguous pixels.
struct TileMap {
  uint32_t W, H;
  uint32_t tiles_x, tiles_y, n_tiles;
  uint32_t shard_rank, shard_count, tiles_per_shard;
  // optional dealing order of the tiles (vx_set_tile_order): position pos = lt * shard_count + rank holds
  // tile perm[pos]; inv is the inverse.  nullptr: pos == tile id (tiles dealt round-robin in row-major order).
  const uint32_t* perm;
  const uint32_t* inv;
};

// Work counters: one record per wave of the launch grid, owned by that wave and updated with a
// plain read-modify-write (launches on a stream are ordered, so no atomics are needed).
// Atomics on shared words were measured to cost ~1.1 ms per 1080p frame (32768 waves x 4
// same-line atomics at ~88 per microsecond) -- three times the march itself.
struct DevCounters {
  unsigned long long samples, slots;
  uint32_t rays, pixels, skips, grads;
  uint32_t last_slots;  // lane slots of the most recent launch: the cost fed back to build_order
  uint32_t gathers;     // 16-byte-per-lane gather wave instructions issued (tuned DVR kernels)
  uint32_t lds_reads;   // LDS tap-read wave instructions (LDS-tile kernels)
  uint32_t tf;          // samples inside the sample range (LUT fetched)
  uint32_t active;      // lane slots that did work (path-traced modes, flush_counts)
  uint32_t pad;
};

// [build] the light grid of shadowed DVR: transmittance toward the directional light at the nodes of a
// lattice of stride s voxels, node (i, j, k) at cell-frame position s * (i, j, k), x fastest
struct ShadowGrid {
  const float* t;   // n[0] * n[1] * n[2] node values
  uint32_t n[3];    // nodes per axis: ceil((extent - 1) / s) + 1
  float inv_s;      // 1 / s (s = 1, 2 or 4: q * inv_s is q / s exactly)
  float glo[3];     // the first and last node per axis whose position lies inside the clip box (vx_api.hip light_march)
  float ghi[3];
  float gmax[3];    // n - 1
};

// counts of one launch (unsigned long long each, zeroed by the host before it)
enum IsoCount { ISO_RAYS = 0, ISO_HITS, ISO_SAMPLES, ISO_REFINE, ISO_SKIPPED, ISO_NCOUNTS };

// The range-skipping table: `bound` holds the upper density bound of every macro cell of the empty-space grid (the intensity
// projections' table, vx_host.hpp compute_projection_bounds); a sample's macro cell is that of its mask cell floor(q) + 1,
// clamped as the projection kernel clamps it (a clamped cell is outside the volume, where every tap reads 0, and the clamped
// macro cell's window holds out-of-grid bricks: its bound is >= 0).
struct IsoBound {
  const float* __restrict__ hi;   // nullptr unless SKIP
  uint32_t sh, md0, md1;          // 3 + level, macro cells per axis x / y
  uint32_t cmax[3];               // extent + 7 per axis
};

// ---- the segment (vx_segment.hpp): masks are brick-major, brick b (x fastest over the brick grid) is 8 x u64, word z, bit y * 8 + x
constexpr uint64_t SEG_COL0 = 0x0101010101010101ull, SEG_COL7 = 0x8080808080808080ull;   // x = 0 / x = 7 of every row
constexpr uint64_t SEG_ROW0 = 0x00000000000000ffull, SEG_ROW7 = 0xff00000000000000ull;   // y = 0 / y = 7

// the statistics and round bookkeeping of one segment (device side; vx_api_segment.hip reads it back whole)
struct SegStats {
  unsigned long long count;
  uint32_t lo[3], hi[3];      // bbox, inclusive
  uint32_t dmin, dmax;        // seg_order_key of the extreme densities
  double sum;                 // written by seg_sum
  uint32_t rounds;            // flood launches with a non-empty worklist
  uint32_t pad;
  unsigned long long visits;  // worklist entries processed
};

struct SegDev {
  uint64_t* pred;        // nb * 8 words
  uint64_t* seg;         // nb * 8 words
  double* partial;       // nb: each brick's float64 sum
  uint32_t* any;         // nb: the predicate has a bit in the brick
  uint32_t* stamp;       // nb: the round + 1 whose worklist the brick was last appended to
  uint32_t* list[2];     // nb each: the worklists of even and odd rounds
  uint32_t* cnt;         // 3: the worklist lengths of rounds r, r + 1, r + 2 (mod 3)
  SegStats* st;
  uint32_t bc[3];
  uint32_t nb;
};

// ---- the distance field (vx_distance.hpp)
// a partial of the field's statistics: the voxels with D2 <= R2, and the largest such D2 over voxels outside the source set with
// idx = the C-order index of the first voxel that attains it, DST_NONE when there is no such voxel
constexpr unsigned long long DST_NONE = ~0ull;
struct DstPartial {
  unsigned long long finite;
  unsigned long long idx;
  float d2;
  uint32_t pad;
};

// ---- the segment store (vx_segstore.hpp)
// a partial of the overlap counts: |A|, |B| and |A & B| over the words a workgroup read
struct SstCount {
  unsigned long long a, b, ab;
};
// the masks of a label map in list order, by value: w[k] = the nb * 8 words of the k-th listed slot, k < n
struct SstSlots {
  const uint64_t* w[VX_SEGMENT_SLOTS];
  uint32_t n;
};

// ---- the histogram (vx_histogram.hpp)
// a brick's share of the moments: the float64 sums of d and d * d and the extreme densities over its voxels of the region
// (0, 0, +inf, -inf for a brick without one); hst_moments reduces the bricks into element 0 of its output
struct HstPartial {
  double sum, sum2;
  float mn, mx;
};
// what a launch of hst_bins needs beside the volume: the region, the bin rule and where the bins go
struct HstParams {
  const uint64_t* mask;      // nb * 8 words of the segment or the slot; nullptr: every voxel of the box
  uint32_t box_lo[3], box_hi[3];
  uint32_t bc[3], nb;
  int32_t rule;              // VxHistRule
  uint32_t bins;             // the number of bins, B or 2^b; `below` is counted at index bins, `above` at bins + 1
  float lo, hi, inv;         // LINEAR
  uint32_t prefix, top_shift, bin_shift, bin_mask;   // KEY: top_shift = 32 - p (32: no prefix), bin_shift = 32 - p - b
  unsigned long long* out;   // bins + 2 counters, zeroed before the launch
  HstPartial* partial;       // nb (MOMENTS only)
};

// ---- the islands (vx_islands.hpp)
// one island while the table is built (device side; the host ranks the rows)
struct IslRow {
  unsigned long long count;
  uint32_t anchor;            // C-order index over (z, y, x) of the island's first voxel
  uint32_t lo[3], hi[3];      // bbox, inclusive
  uint32_t pad;
};

struct IslHdr {
  uint32_t roots;      // isl_scan: the number of islands
  uint32_t seed_row;   // isl_seed_row: the row of the seed voxel, ISL_NONE when it is not set
  uint32_t retries;    // isl_merge: failed compare-exchanges (a probe figure; not part of any result)
  uint32_t pad;
};

struct IslDev {
  uint32_t* lab;       // nb * 512
  uint32_t* nroots;    // nb
  uint32_t* off;       // nb
  IslHdr* hdr;
  IslRow* rows;        // cap
  uint32_t* newlab;    // cap: the label (rank + 1) of a row, 0 when the op dropped it
  uint32_t cap;
};

// ---- the mesh (vx_mesh.hpp)
struct MeshStats {
  unsigned long long verts, quads, active_blocks;
  uint32_t lo[3], hi[3];   // bbox of the active cells as cell + 1 (cells start at -1)
};

struct MeshDev {
  uint64_t* inside;   // nb * 8 words
  uint64_t* act;      // ncb * 8 words: the active cells of every cell block
  uint2* vq;          // ncb: {vertices, quads} of the block
  uint2* off;         // ncb: their exclusive prefix sums
  uint2* part;        // np: the sums of each workgroup of mesh_active (256 blocks)
  uint2* poff;        // np: their exclusive prefix sums
  MeshStats* st;
  uint32_t bc[3], cb[3];   // bricks, cell blocks (= bricks + 1) per axis
  uint32_t nb, ncb, np;
};

}  // namespace vx
