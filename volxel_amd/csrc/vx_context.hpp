// vx_context.hpp -- the context behind the C ABI of include/volxel_hip.h, once, for every unit of the host layer
// (vx_api.hip, vx_api_volume.hip, vx_api_view.hip, vx_api_segment.hip, vx_api_mesh.hip): VxContext and what it is made
// of, the helpers of device groups, the dispatch helpers from a run-time value to a template argument, and the parameter
// checks the entry points of several units share.  Host only: no kernel and no device code, and no kernel header is
// included -- the plain structs the context holds by value come from vx_types.hpp.
#pragma once

#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <optional>
#include <string>
#include <type_traits>
#include <vector>

#include "vx_host.hpp"
#include "vx_types.hpp"

namespace vx __attribute__((visibility("hidden"))) {

struct EventPair {
  hipEvent_t a, b;
  bool merge = false;      // interval of a merge_results launch (reported apart, VxCounters.merge_ms)
};

// The diagnostic switches of the environment, read once by vx_create (none changes a result bit).
struct Switches {
  int dvr_variant = -1;            // VX_DVR_KERNEL=generic: 0, the DVR modes on render_generic; -1: the tuned kernels
  bool dvr_fuse = true;            // VX_DVR_FUSE=0: no kernel folds the running mean; merge_results blends every multi-frame launch
  bool ray_shortcuts = true;       // VX_RAY_SHORTCUTS=0: the per-ray divisions themselves (DevVolume::ray_flags = 0)
  std::optional<uint64_t> cellquad_max_bytes;   // VX_AUTO_CELLQUAD_MAX_BYTES: AUTO's budget for the cellquad layout (ensure_layout)
  uint32_t seg_check_max = 64;     // VX_SEG_CHECK_MAX (1 .. 4096): the largest batch of flood rounds between read-backs (vx_segment)
  bool dvr_miss = true;            // VX_DVR_MISS=0: no multi-frame DVR launch is split; every block runs the LDS-window kernel
  uint32_t dist_lds_bytes = 65536; // VX_DIST_LDS_BYTES (256 .. 65536): the LDS a tile of the distance line passes may take (its width follows)
};

// ---- the tables a launch derives from the params and the uploads ---------------------------------------------------------
// The skip mask, the projection bounds, the local majorants and the light grid share one cache rule: a table is rebuilt
// before a launch that reads it when an upload marked it stale or when its key -- the bits of the params it is built from,
// listed once in its key function -- differs from the key of the last build.  A camera move rebuilds none of them but the
// split of a multi-frame DVR launch (miss_key: host arithmetic and one asynchronous copy, no wait on the stream).

// the bits of 4-byte params and param arrays, in order
template <class... T>
std::array<uint32_t, (sizeof(T) + ...) / 4> key_of(const T&... v) {
  static_assert(((sizeof(T) % 4 == 0) && ...), "key fields are 4-byte values");
  std::array<uint32_t, (sizeof(T) + ...) / 4> k{};
  uint32_t* o = k.data();
  ((memcpy(o, &v, sizeof v), o += sizeof v / 4), ...);
  return k;
}
inline auto skip_key(const VxParams& p) { return key_of(p.volume_density_scale, p.volume_inv_maj, p.sample_range); }
inline auto proj_key(const VxParams& p) { return key_of(p.volume_density_scale, p.volume_inv_maj, p.render_mode); }
inline auto iso_key(const VxParams& p) { return key_of(p.volume_density_scale, p.volume_inv_maj); }
inline auto lmaj_key(const VxParams& p) { return key_of(p.volume_density_scale, p.volume_inv_maj, p.volume_maj, p.sample_range); }
inline auto shadow_key(const VxParams& p) {
  return key_of(p.light_dir, p.density_transform_inv, p.volume_aabb_min, p.volume_aabb_max, p.volume_maj, p.volume_inv_maj,
                p.volume_density_scale, p.sample_range, p.dvr_step_voxels, p.dvr_ert_tau, p.dvr_max_steps, p.dvr_shadow_stride);
}
// the split of a multi-frame DVR launch (classify_miss_blocks): the matrices the rays use, the clip box, the image, the shard
// -- a camera move DOES rebuild this one, ahead of the next multi-frame launch (host arithmetic on eight corners and a
// frame's blocks); the tile map marks it stale itself
inline auto miss_key(const VxParams& p) {
  return key_of(p.camera_view_inv, p.camera_proj_inv, p.camera_ortho, p.volume_aabb_min, p.volume_aabb_max, p.res, p.shard_rank,
                p.shard_count);
}

template <auto KEY>
struct DerivedTable {
  bool stale = true;                      // never built, an upload since the last build, or a rebuild that failed
  decltype(KEY(VxParams{})) key{};        // KEY of the params of the last build
  bool current(const VxParams& p) const { return !stale && KEY(p) == key; }
  void built(const VxParams& p) {
    key = KEY(p);
    stale = false;
  }
};

}  // namespace vx

using namespace vx;   // (VxContext is the C ABI's global type; it names the library's own types unqualified)

struct VxContext : VxCore {   // (device, the stream the launches go to, the last error: vx_host.hpp)
  hipStream_t own_stream = nullptr;
  hipDeviceProp_t prop;

  // Everything that describes the resident volume: vx_upload_volume drops it as a whole (free_volume), so a buffer or a flag
  // that must not outlive the volume belongs here and needs no line anywhere else.
  struct Volume {
    bool has_volume = false;
    DevVolume dv{};
    DevBuf<void> cq_alloc, bf_alloc;
    DevBuf<void> bu_alloc;     // bricku8 codes (+ one zero unit)
    DevBuf<void> bur_alloc;    // bricku8 per-brick {min, max - min} (+ the {0, 0} entry of the zero unit)
    // the derived tables (their device arrays below, outside: rebuilt before the next launch that reads them)
    DerivedTable<skip_key> skip_table;
    DerivedTable<proj_key> proj_table;
    DerivedTable<lmaj_key> lmaj_table;
    DerivedTable<shadow_key> shadow_table;
    DerivedTable<iso_key> iso_table;
    DevBuf<float> lmaj_dev;    // default mode: local-majorant table (DevVolume::lmaj)
    // shadowed DVR: the light grid (vx_shadow.hpp)
    DevBuf<float> shadow_dev;
    ShadowGrid shadow{};       // what the last build made (t == nullptr: none since the last upload)
    // segmentation (vx_segment): one allocation for the masks, flags, stamps, worklists, partial sums and statistics of the
    // brick grid (ensure_segment); the packed mask of vx_segment_read_mask / vx_segment_write_mask grows on demand
    DevBuf<void> seg_alloc;
    SegDev seg{};
    bool seg_valid = false;        // a segment of the resident volume is current
    bool seg_pred_valid = false;   // SegDev::pred holds the predicate of a vx_segment / vx_segment_threshold on this volume
    int seg_view = VX_SEGVIEW_OFF;   // vx_set_segment_view; OFF again after an upload
    DevBuf<uint8_t> seg_bytes;
    // segment edits: two scratch masks and the fill's flags, allocated by the first vx_segment_edit (ensure_segedit)
    DevBuf<void> sed_alloc;
    uint64_t* sed_mask[2] = {nullptr, nullptr};
    uint32_t* sed_any = nullptr;
    // islands (vx_segment_islands): the labels (one u32 per voxel, brick-major), the root counts and their scan in one
    // allocation made by the first call; the rows and their labels grow to the largest table; the ranked table lives on the
    // host; the dense label volume is allocated by the first vx_islands_read_labels
    DevBuf<void> isl_alloc, isl_rows_alloc;
    IslDev isl{};
    bool isl_valid = false;    // the table and the labels describe the current segment
    std::vector<VxIsland> isl_table;
    DevBuf<uint32_t> isl_dense;
    // distances (vx_segment_distance, vx_segment_margin): the D2 field, one fp32 per voxel, and the partials of its statistics,
    // allocated by the first call (ensure_distance)
    DevBuf<float> dist_field;
    DevBuf<DstPartial> dist_partials;
    bool dist_valid = false;   // the field is the last vx_segment_distance's and the mask has not changed since
    // the segment store (vx_segment_store .. vx_segments_labelmap): a slot is an allocation of its own of nb * 8 words, made by
    // the first store to it (p != nullptr: occupied); the partials of the overlap counts and the dense label map (1 B per voxel,
    // with the count of overlapping voxels behind it) are allocated by the first call that needs them
    DevBuf<uint64_t> slots[VX_SEGMENT_SLOTS];
    DevBuf<SstCount> sst_partials;
    DevBuf<uint8_t> sst_labels;
    DevBuf<unsigned long long> sst_overlaps;
    // histograms (vx_histogram): the 64-bit bins with `below` and `above` behind them, and the bricks' partial moments with
    // their total behind them (24 B per brick), allocated by the first call that needs them
    DevBuf<unsigned long long> hst_bins;
    DevBuf<HstPartial> hst_partials;
    // meshes (vx_mesh_extract): one allocation for the inside words, the active words, the counts and their scans
    // (ensure_mesh); the vertex / cell buffers (3 values per vertex, grown together) and the triangles grow to the largest mesh
    DevBuf<void> mesh_alloc;
    MeshDev mesh{};
    bool mesh_valid = false;   // a mesh of the resident volume is current
    DevBuf<float> mesh_verts;
    DevBuf<int32_t> mesh_cells;
    DevBuf<uint32_t> mesh_tris;
    uint64_t mesh_nv = 0, mesh_nt = 0;
  } vol;
  std::vector<void*> vol_allocs;     // the uploaded arrays DevVolume points to (free_volume)
  int layout = VX_LAYOUT_AUTO;       // what the host asked for (vx_set_layout); eff_layout() is what a launch samples
  bool auto_no_cq = false;           // AUTO: no cellquad layout (index range or memory budget): `default` / `no_dda` take primary_layout
  bool auto_no_bf = false;           // AUTO: too large for brickf32 as well (everything uses REFERENCE)

  // ---- what survives an upload ----
  // transfer function
  DevBuf<float4> tf;
  uint32_t tf_len = 0;
  std::vector<float> tf_host;

  std::vector<uint32_t> range_host;   // packed (min16<<16)|max16 per brick
  DevBuf<uint32_t> skip_dev;          // exact empty-space skipping (DVR): macro-cell bitmask
  DevBuf<float> proj_dev;             // range skipping of the intensity projections: one density bound per macro cell

  DevBuf<unsigned long long> fold_dev;   // the totals of fold_records

  DevBuf<unsigned long long> shadow_count_dev;   // light-march samples of the last light-grid build
  StageTimer<1> shadow_timer;
  uint64_t shadow_builds = 0;

  // params
  VxParams params{};
  bool has_params = false;

  // framebuffers
  uint32_t W = 0, H = 0;
  TileMap tm{};
  DevBuf<float4> slab;
  size_t slab_quads = 0;
  DevBuf<float4> image;
  DevBuf<float4> env_tex;      // environment map, GL row order
  DevBuf<float> env_imp;       // importance pyramid
  DevBuf<float4> env_impq;     // the pyramid as sibling quads (sample_environment)
  float env_avg_w = 0.0f;
  uint32_t env_w = 0, env_h = 0;
  DevBuf<uchar4> display;
  DevBuf<uint32_t> tile_perm;  // vx_set_tile_order: position -> tile, tile -> position (2 * n_tiles)
  uint32_t tile_perm_n = 0;
  std::vector<uint32_t> tile_perm_host;   // position -> tile as the device holds it (empty: pos == tile id)
  // The split of a multi-frame DVR launch of the LDS-window kernel (ensure_miss_split): per logical block of a frame, 1 = it goes to
  // render_dvr_miss -- no ray of its pixels can hit the clip box (`proved` of them), or it lies outside the shard's tiles or
  // the image, where either kernel returns at once; the two halves of `order`, split_order's stable partition.
  struct MissSplit {
    DerivedTable<miss_key> table;     // stale: never built, or the tile map changed
    std::vector<uint8_t> flags_host;
    DevBuf<uint8_t> flags;
    DevBuf<uint32_t> order_heavy, order_miss;
    uint32_t blocks = 0;              // frame_blocks of the build
    uint32_t n_miss = 0, proved = 0;
    bool split_stale = true;          // `order` or the flags changed since split_order ran
    uint32_t last_heavy = 0, last_miss = 0;   // blocks per frame slot the last render launch gave each kernel
    // the flags cross to the device from two pinned buffers used in turn: the copy is asynchronous on the context's stream, and
    // a buffer is rewritten only behind the event of its last copy (two builds back: complete long since, no stall)
    struct Stage {
      uint8_t* p = nullptr;
      size_t cap = 0;
      hipEvent_t done = nullptr;
      bool pending = false;
    } stage[2];
    int next_stage = 0;
    MissSplit() = default;
    MissSplit(const MissSplit&) = delete;
    MissSplit& operator=(const MissSplit&) = delete;
    ~MissSplit() {
      for (Stage& st : stage) {
        if (st.p) (void)hipHostFree(st.p);
        if (st.done) (void)hipEventDestroy(st.done);
      }
    }
  } miss;

  // counters / timing
  DevBuf<DevCounters> dc;      // one record per wave of the largest launch grid
  size_t dc_waves = 0;
  DevBuf<uint32_t> order;      // launch permutation of the DVR kernel (build_order), dc_waves/4 entries
  int tex_checked_res[2] = {-1, -1};  // DevVolume::ray_flags: the resolution (pixel + 0.5) / res was last tried against its reciprocal form
  bool tex_by_reciprocal[2] = {false, false};
  Switches sw;
  int order_builds_left = 2;   // rebuild the order after the first frames that follow a change
  VxCounters base{};           // totals folded in when the record array is reallocated
  std::vector<EventPair> free_events, pending_events;
  double kernel_ms = 0.0, last_kernel_ms = 0.0, merge_ms = 0.0;
  uint64_t launches = 0, frames = 0, merge_launches = 0;
  uint32_t min_launch_frames = 0, max_launch_frames = 0;   // what the launches since the last reset covered
  hipStream_t aux_stream = nullptr;   // layout builds of an upload, overlapped with the atlas copy
  double upload_seconds = 0.0;        // wall time of the last vx_upload_volume (copies + layout build)
  uint64_t upload_host_bytes = 0;     // host bytes it moved over PCIe
  int upload_pinned = 0;              // whether the atlas could be pinned in place
  void note_launch(uint32_t n) {
    launches += 1;
    frames += n;
    min_launch_frames = (min_launch_frames == 0 || n < min_launch_frames) ? n : min_launch_frames;
    max_launch_frames = n > max_launch_frames ? n : max_launch_frames;
  }
  // per-frame result slabs and counter records of multi-frame launches (vx_render_frames), pipe_slots of each in ONE
  // allocation (slot i at i * pipe_quads / i * pipe_waves)
  DevBuf<float4> pipe_result_pool;
  DevBuf<DevCounters> pipe_dc_pool;
  size_t pipe_quads = 0, pipe_waves = 0;
  uint32_t pipe_slots = 0;
  // the slab table the detile kernel reads (one entry per shard, on this device); slab_table_host is what it holds
  DevBuf<const float4*> slab_table;
  std::vector<const float4*> slab_table_host;
  // device group (vx_create_group): member i renders shard i of members.size(); empty for a plain context
  std::vector<VxContext*> members;
  hipEvent_t done = nullptr;   // a member's: recorded after its last render, waited on by the display stream
  // slices (vx_slice): the output buffers, grown to the largest slice, and the facts of the last slice
  DevBuf<float> slice_values;
  DevBuf<uchar4> slice_rgba;
  StageTimer<1> slice_timer;
  uint64_t slice_samples = 0;
  // isosurfaces (vx_isosurface): the output buffers, grown to the largest window; the upper density bounds of range skipping
  // (its own copy of the projections' table, so that MIP's bookkeeping is never disturbed); the counts of the last call
  DevBuf<float4> iso_rgba, iso_hit;
  DevBuf<float> iso_bound_dev;
  IsoBound iso_bound{};
  DevBuf<unsigned long long> iso_count_dev;   // ISO_NCOUNTS
  StageTimer<1> iso_timer;
  uint64_t iso_counts[ISO_NCOUNTS] = {};
  // the segment chain: the overlay of vx_slice_segment_mask, grown to the largest slice; the last vx_segment's result; the
  // timers and launch counts the *_stats entry points report.  sed_timer / sed_launches belong to every call that rewrites
  // the mask outright (vx_segment_edit, vx_segment_write_mask, vx_segment_threshold: vx_segment_edit_stats), not to the
  // edit scratch.
  DevBuf<uint8_t> seg_ov;
  VxSegmentResult seg_res{};
  StageTimer<3> seg_timer;
  StageTimer<2> sed_timer;
  uint32_t sed_launches = 0;
  StageTimer<7> isl_timer;
  uint32_t isl_launches = 0;
  StageTimer<3> mesh_timer;
  uint32_t mesh_launches = 0;
  // distances: two rounds of (x, y, z, compare / reduce) and the statistics of a margin's mask; dst_ms sums the rounds per pass
  StageTimer<9> dst_timer;
  double dst_ms[4] = {};
  uint32_t dst_launches = 0;
  // histograms: the histogram pass and the moments' reduction of the last vx_histogram
  StageTimer<2> hst_timer;
  uint32_t hst_launches = 0;
};

namespace vx __attribute__((visibility("hidden"))) {

inline bool is_group(const VxContext* c) { return !c->members.empty(); }

// every entry point that touches the device first makes the context's device current for the
// calling thread (a host with several contexts / devices must not depend on its own hipSetDevice)
#define VX_DEV(ctx) VX_HIP(ctx, hipSetDevice((ctx)->device))

// calls f(std::integral_constant<int, LAYOUT_*>) for the device layout `lay` (the path kernels and the tile-cost probe
// sample brickf32, cellquad, or -- for every other layout -- the reference textures)
template <class F>
inline void with_layout(int lay, F&& f) {
  if (lay == VX_LAYOUT_BRICKF32) f(std::integral_constant<int, LAYOUT_BF>{});
  else if (lay == VX_LAYOUT_CELLQUAD) f(std::integral_constant<int, LAYOUT_CQ>{});
  else f(std::integral_constant<int, LAYOUT_REF>{});
}

// calls f(std::integral_constant<bool, b>)
template <class F>
inline void with_bool(bool b, F&& f) {
  if (b) f(std::true_type{});
  else f(std::false_type{});
}
// calls f(std::integral_constant<int, 6 or 26>) for a checked connectivity (the flood, the edit steps, the islands)
template <class F>
inline void with_conn(int conn, F&& f) {
  if (conn == 26) f(std::integral_constant<int, 26>{});
  else f(std::integral_constant<int, 6>{});
}

inline bool proj_mode(int m) { return m == VX_MODE_MIP || m == VX_MODE_MINIP; }

// The device layout the kernels of the current render mode sample.  VX_LAYOUT_AUTO (default): the DVR modes march
// the brickf32 layout through LDS windows (vx_dvr_lds.hpp: fastest, 4 bytes per voxel), `default` and `no_dda`
// gather from cellquad (two 16-byte loads per trilinear look-up instead of eight bounds-checked taps), `raymarch`
// reads its single nearest tap from brickf32.
inline int primary_layout(const VxContext* c) {
  if (c->layout != VX_LAYOUT_AUTO) return c->layout;
  return c->auto_no_bf ? VX_LAYOUT_REFERENCE : VX_LAYOUT_BRICKF32;
}
inline int eff_layout(const VxContext* c) {
  if (c->layout != VX_LAYOUT_AUTO) return c->layout;
  const int m = c->has_params ? c->params.render_mode : VX_MODE_DVR;
  // raymarch takes ONE nearest tap per sample (common.glsl:72-76): the 4-byte-per-voxel bricks serve it better than
  // the 18-byte-per-voxel quads, and the layout is resident already
  if (m == VX_MODE_DVR || m == VX_MODE_DVR_PHONG || m == VX_MODE_RAYMARCH || proj_mode(m)) return primary_layout(c);
  // `default` / `no_dda`: cellquad (18 B / voxel) while the volume is inside its index range and the build fits the device
  // memory budget (ensure_layout); beyond that the fp32 bricks that are resident anyway -- eight taps per look-up, measured
  // 1.4x / 2.0x slower than cellquad and 2.0x / 2.2x faster than the reference textures on the 1024^3 volume at 3840x2160
  // (profiles/r04_layouts_1024.txt) -- and the reference textures only when neither native layout can index the volume
  return c->auto_no_cq ? primary_layout(c) : VX_LAYOUT_CELLQUAD;
}

// The layout a slice samples: what is resident at the time of the call -- brickf32, else cellquad, else the reference textures
// (same bits on all three).  Not eff_layout: under AUTO it follows the render mode, and for `default` / `no_dda` it names
// cellquad before the first render of such a mode has built it; under bricku8 the slice reads the reference textures.
inline int slice_layout(const VxContext* c) {
  if (c->vol.dv.bf) return VX_LAYOUT_BRICKF32;
  if (c->vol.dv.cq) return VX_LAYOUT_CELLQUAD;
  return VX_LAYOUT_REFERENCE;
}

// ---- device groups (vx_create_group): the entry points fan out to the members, read member 0, or gather --------
// a member's failure, reported on the group handle with the member's index and device
inline int member_fail(VxContext* g, size_t i, int rc) {
  char head[64];
  snprintf(head, sizeof head, "member %zu (device %d): ", i, g->members[i]->device);
  g->err = head + g->members[i]->err;
  return rc;
}
template <class F>
inline int fan_out(VxContext* g, F&& f) {
  for (size_t i = 0; i < g->members.size(); ++i)
    if (int rc = f(g->members[i], i)) return member_fail(g, i, rc);
  return VX_OK;
}
inline int on_member0(VxContext* g, int rc) { return rc ? member_fail(g, 0, rc) : VX_OK; }
inline int refuse_group(VxContext* g, const char* fn, const char* why) {
  VX_FAIL(g, VX_ERR_INVALID, "%s: not for a device group (%s)", fn, why);
}

// ---- the parameter checks the slice and segment entry points share -------------------------------------------------------
// Each takes the entry point's name: the refusals read "<entry point>: ..." as they always did.

// the preamble: a volume, the params, and the entry point's own argument
inline int check_ready(VxContext* c, const char* fn, const void* arg, const char* arg_name) {
  if (!c->vol.has_volume) VX_FAIL(c, VX_ERR_NO_VOLUME, "%s: no volume uploaded", fn);
  if (!c->has_params)
    VX_FAIL(c, VX_ERR_INVALID, "%s: vx_set_params first (volume_density_scale and volume_inv_maj come from it)", fn);
  if (!arg) VX_FAIL(c, VX_ERR_INVALID, "%s: %s is NULL", fn, arg_name);
  return VX_OK;
}
inline int check_slice_size(VxContext* c, const char* fn, const VxSliceParams* sp) {
  for (int i = 0; i < 2; ++i)
    if (sp->size[i] < 1u || sp->size[i] > 16384u) VX_FAIL(c, VX_ERR_INVALID, "%s: size[%d] = %u outside 1 .. 16384", fn, i, sp->size[i]);
  if (sp->slab_samples < 1u || sp->slab_samples > 4096u)
    VX_FAIL(c, VX_ERR_INVALID, "%s: slab_samples = %u outside 1 .. 4096", fn, sp->slab_samples);
  return VX_OK;
}
inline int check_slice_frame(VxContext* c, const char* fn, const VxSliceParams* sp) {
  const struct { const char* name; const float* v; } vecs[4] = {{"origin", sp->origin}, {"du", sp->du}, {"dv", sp->dv}, {"dn", sp->dn}};
  for (const auto& e : vecs)
    for (int i = 0; i < 3; ++i)
      if (!std::isfinite(e.v[i])) VX_FAIL(c, VX_ERR_INVALID, "%s: %s[%d] is not finite", fn, e.name, i);
  return VX_OK;
}
inline int check_band(VxContext* c, const char* fn, float lo, float hi) {
  if (!std::isfinite(lo)) VX_FAIL(c, VX_ERR_INVALID, "%s: lo is not finite", fn);
  if (!std::isfinite(hi)) VX_FAIL(c, VX_ERR_INVALID, "%s: hi is not finite", fn);
  if (lo > hi) VX_FAIL(c, VX_ERR_INVALID, "%s: lo = %g > hi = %g", fn, (double)lo, (double)hi);
  return VX_OK;
}
inline int check_connectivity(VxContext* c, const char* fn, int conn) {
  if (conn != 6 && conn != 26) VX_FAIL(c, VX_ERR_INVALID, "%s: connectivity = %d is not 6 or 26", fn, conn);
  return VX_OK;
}
inline int check_seed(VxContext* c, const char* fn, const uint32_t seed[3]) {
  for (int a = 0; a < 3; ++a)
    if (seed[a] >= c->vol.dv.extent[a])
      VX_FAIL(c, VX_ERR_INVALID, "%s: seed[%d] = %u outside the index extent %u", fn, a, seed[a], c->vol.dv.extent[a]);
  return VX_OK;
}
// the voxel box [box_lo, box_hi] with VX_SEGMENT_BOX_END resolved, inside the index extent
struct VoxelBox {
  uint32_t lo[3], hi[3];
};
inline int check_box(VxContext* c, const char* fn, const uint32_t box_lo[3], const uint32_t box_hi[3], VoxelBox* b) {
  const uint32_t* E = c->vol.dv.extent;
  for (int a = 0; a < 3; ++a) {
    b->lo[a] = box_lo[a];
    b->hi[a] = box_hi[a] == VX_SEGMENT_BOX_END ? E[a] - 1u : box_hi[a];
    if (b->lo[a] > b->hi[a] || b->hi[a] >= E[a])
      VX_FAIL(c, VX_ERR_INVALID, "%s: box axis %d [%u, %u] is empty or outside the index extent %u", fn, a, box_lo[a], box_hi[a], E[a]);
  }
  return VX_OK;
}
// bytes of the packed mask (1 bit per voxel) a caller hands over or receives
inline int check_mask_bytes(VxContext* c, const char* fn, uint64_t nbytes, size_t* want) {
  const uint32_t* E = c->vol.dv.extent;
  *want = (size_t)E[0] * E[1] * E[2] / 8u;
  if (nbytes != *want)
    VX_FAIL(c, VX_ERR_INVALID, "%s: nbytes = %llu, the mask of %u x %u x %u voxels is %zu bytes", fn, (unsigned long long)nbytes, E[0],
            E[1], E[2], *want);
  return VX_OK;
}

// ---- the functions one unit defines and another calls (hidden like the rest of this namespace: the library exports none) -----
// defined in vx_api.hip, which knows whether a launch has an LDS-window kernel; also called by vx_isosurface (vx_api_view.hip)
int check_segment_view(VxContext* c, const char* fn, bool iso);
// defined in vx_api_volume.hip.  free_volume drops the resident volume and everything derived from it (the caller has made the
// context's device current).  ensure_layout makes `layout` (brickf32 or cellquad) resident beside what is there, for a launch
// prepare_render found to sample it; VX_OK without it where the launch has another way: a volume beyond the layout's index range, or
// AUTO's cellquad beyond its memory budget (then auto_no_cq is set and eff_layout steps down).
void free_volume(VxContext* c);
int ensure_layout(VxContext* c, int layout);

}  // namespace vx
