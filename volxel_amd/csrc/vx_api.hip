// vx_api.hip -- the render unit of libvolxel_hip.so's host layer (the C ABI of include/volxel_hip.h; units: DESIGN.md section
// 4.1): contexts and device groups, the transfer-function and environment uploads, the derived tables, the launch plan,
// rendering, read-back, counters, probes and test hooks.  Every render_* kernel is instantiated here, so this unit's listing (vx_api.s) holds them all.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "vx_dvr.hpp"
#include "vx_dvr_lds.hpp"
#include "vx_dvr_miss.hpp"
#include "vx_kernels.hpp"
#include "vx_shadow.hpp"
#include "vx_projection.hpp"
#include "vx_context.hpp"

using namespace vx;

namespace {

thread_local std::string g_create_error;

// VX_DVR_MISS alone: vx_create reads it with the others, and the classifier's test hook -- which has no context to hold a
// Switches -- reads this one variable and nothing else
bool dvr_miss_switch() {
  const char* v = getenv("VX_DVR_MISS");
  return !(v && atoi(v) == 0);
}
// the only place that reads the other switches from the environment (vx_create)
Switches read_switches() {
  Switches sw;
  if (const char* v = getenv("VX_DVR_KERNEL"); v && !strcmp(v, "generic")) sw.dvr_variant = 0;
  if (const char* v = getenv("VX_DVR_FUSE")) sw.dvr_fuse = atoi(v) != 0;
  if (const char* v = getenv("VX_RAY_SHORTCUTS"); v && atoi(v) == 0) sw.ray_shortcuts = false;
  if (const char* v = getenv("VX_AUTO_CELLQUAD_MAX_BYTES")) sw.cellquad_max_bytes = strtoull(v, nullptr, 10);
  if (const char* v = getenv("VX_SEG_CHECK_MAX")) sw.seg_check_max = (uint32_t)std::min(std::max(atoi(v), 1), 4096);
  if (const char* v = getenv("VX_DIST_LDS_BYTES")) sw.dist_lds_bytes = (uint32_t)std::min(std::max(atoi(v), 256), 65536);
  sw.dvr_miss = dvr_miss_switch();
  return sw;
}

static void drain_events(VxContext* c) {
  for (auto& e : c->pending_events) {
    (void)hipEventSynchronize(e.b);
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, e.a, e.b) == hipSuccess) {
      if (e.merge) {
        c->merge_ms += ms;
      } else {
        c->kernel_ms += ms;
        c->last_kernel_ms = ms;
      }
    }
    e.merge = false;
    c->free_events.push_back(e);
  }
  c->pending_events.clear();
}

static void update_tilemap(VxContext* c) {
  TileMap& t = c->tm;
  t.W = c->W;
  t.H = c->H;
  t.tiles_x = (c->W + VX_SHARD_TILE - 1) / VX_SHARD_TILE;
  t.tiles_y = (c->H + VX_SHARD_TILE - 1) / VX_SHARD_TILE;
  t.n_tiles = t.tiles_x * t.tiles_y;
  t.shard_count = c->has_params && c->params.shard_count > 0 ? (uint32_t)c->params.shard_count : 1u;
  t.shard_rank = c->has_params ? (uint32_t)c->params.shard_rank : 0u;
  t.tiles_per_shard = (t.n_tiles + t.shard_count - 1) / t.shard_count;
  if (c->tile_perm && c->tile_perm_n != t.n_tiles) {  // the order belongs to another tile grid
    c->tile_perm.reset();
    c->tile_perm_n = 0;
  }
  if (!c->tile_perm) c->tile_perm_host.clear();
  c->miss.table.stale = true;   // blocks map to other pixels
  t.perm = c->tile_perm;
  t.inv = c->tile_perm ? c->tile_perm + t.n_tiles : nullptr;
}

static int alloc_framebuffers(VxContext* c) {
  if (c->order && c->dc_waves) {  // the launch permutation belongs to the old grid: back to identity
    std::vector<uint32_t> ident(c->dc_waves / 4);
    for (size_t i = 0; i < ident.size(); ++i) ident[i] = (uint32_t)i;
    VX_HIP(c, hipMemcpy(c->order, ident.data(), ident.size() * 4, hipMemcpyHostToDevice));
    c->order_builds_left = 2;
    c->miss.split_stale = true;
  }
  // grow-only: the low-resolution preview (viewer.ts:1167-1188) resizes twice per restart
  update_tilemap(c);
  c->slab_quads = (size_t)c->tm.tiles_per_shard * 4096u;
  if (c->slab_quads == 0) return VX_OK;
  size_t px = (size_t)c->W * c->H;
  if (int rc = c->slab.ensure(c, c->slab_quads)) return rc;
  if (int rc = c->image.ensure(c, px)) return rc;
  if (int rc = c->display.ensure(c, px)) return rc;
  VX_HIP(c, hipMemsetAsync(c->slab, 0, c->slab_quads * sizeof(float4), c->stream));
  return VX_OK;
}

// the device table: the bound the mode tests (hi for MIP, lo for MinIP), one float per macro cell
static int rebuild_projection_bounds(VxContext* c) {
  const VxParams& p = c->params;
  c->vol.proj_table.stale = true;   // until this build is complete
  std::vector<float> lohi;
  int level = 1;
  uint32_t md[3];
  compute_projection_bounds(p, c->range_host.data(), c->vol.dv.bc, c->vol.dv.extent, lohi, level, md);
  const size_t n = lohi.size() / 2;
  std::vector<float> one(n);
  const int which = p.render_mode == VX_MODE_MINIP ? 0 : 1;
  for (size_t i = 0; i < n; ++i) one[i] = lohi[2 * i + which];
  if (int rc = c->proj_dev.alloc(c, n)) return rc;
  VX_HIP(c, hipMemcpyAsync(c->proj_dev, one.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  // the macro-cell grid the kernel indexes: the empty-space grid's level and dims (a function of the extent alone, so the
  // same values rebuild_skip_mask sets for this volume)
  c->vol.dv.skip_level = (uint32_t)level;
  for (int a = 0; a < 3; ++a) c->vol.dv.skip_dims[a] = md[a];
  c->vol.proj_table.built(p);
  return VX_OK;
}

// the local majorants of the default mode, tabulated on the device with the operations of Frame::local_majorant
static int rebuild_local_majorants(VxContext* c) {
  const VxParams& p = c->params;
  c->vol.lmaj_table.stale = true;   // until this build is complete
  const size_t n = 4 * (size_t)c->vol.dv.bc[0] * c->vol.dv.bc[1] * c->vol.dv.bc[2] + 1;
  if (int rc = c->vol.lmaj_dev.ensure(c, n)) return rc;
  DevVolume dv = c->vol.dv;
  dv.lmaj = nullptr;
  hipLaunchKernelGGL(build_local_majorants, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, p, dv, c->tf,
                     c->tf_len, c->vol.lmaj_dev);
  VX_HIP(c, hipGetLastError());
  c->vol.dv.lmaj = c->vol.lmaj_dev;
  c->vol.dv.lmaj_cells = (uint32_t)(n - 1);
  c->vol.lmaj_table.built(p);
  return VX_OK;
}

static int rebuild_skip_mask(VxContext* c) {
  const VxParams& p = c->params;
  c->vol.skip_table.stale = true;   // until this build is complete
  std::vector<uint32_t> bits;
  int level = 1;
  uint32_t md[3];
  compute_skip_mask(p, c->range_host.data(), c->vol.dv.bc, c->vol.dv.extent, c->tf_host.data(), c->tf_len, bits, level, md);
  if (int rc = c->skip_dev.alloc(c, bits.size())) return rc;
  VX_HIP(c, hipMemcpyAsync(c->skip_dev, bits.data(), bits.size() * 4, hipMemcpyHostToDevice, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  c->vol.dv.skip_bits = c->skip_dev;
  c->vol.dv.skip_level = (uint32_t)level;
  c->vol.dv.skip_words = (uint32_t)bits.size();
  for (int a = 0; a < 3; ++a) c->vol.dv.skip_dims[a] = md[a];
  c->vol.skip_table.built(p);
  return VX_OK;
}

// fold every record array (accumulator slot and the multi-frame slots) into c->base on the device and zero it
static int fold_counters(VxContext* c) {
  if (!c->dc || !c->dc_waves) return VX_OK;
  if (int rc = c->fold_dev.ensure(c, 10)) return rc;
  hipLaunchKernelGGL(zero_totals, dim3(1), dim3(10), 0, c->stream, c->fold_dev);
  auto fold = [&](DevCounters* recs, size_t n) {
    const unsigned blocks = (unsigned)std::min<size_t>((n + 255) / 256, 2048);
    hipLaunchKernelGGL(fold_records, dim3(blocks), dim3(256), 0, c->stream, recs, n, c->fold_dev);
  };
  fold(c->dc, c->dc_waves);
  if (c->pipe_dc_pool) fold(c->pipe_dc_pool, c->pipe_slots * c->pipe_waves);
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipStreamSynchronize(c->stream));
  unsigned long long h[10];
  VX_HIP(c, hipMemcpy(h, c->fold_dev, sizeof h, hipMemcpyDeviceToHost));
  c->base.samples += h[0];
  c->base.lane_slots += h[1];
  c->base.rays += h[2];
  c->base.pixels += h[3];
  c->base.skip_steps += h[4];
  c->base.grad_samples += h[5];
  c->base.gathers += h[6];
  c->base.lds_reads += h[7];
  c->base.tf_samples += h[8];
  c->base.active_lane_slots += h[9];
  return VX_OK;
}

static int ensure_counters(VxContext* c, size_t waves) {
  if (waves <= c->dc_waves) return VX_OK;
  VX_HIP(c, hipStreamSynchronize(c->stream));
  int rc = fold_counters(c);
  if (rc) return rc;
  c->dc_waves = 0;
  if (int rc = c->dc.alloc(c, waves)) return rc;
  // on the context's stream: it is a non-blocking stream, a fill on the null stream is not ordered with the launches
  // that follow (seen under rocprofv3's counter collection: the late fill wiped the records of a launch)
  VX_HIP(c, hipMemsetAsync(c->dc, 0, waves * sizeof(DevCounters), c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  c->dc_waves = waves;
  {
    std::vector<uint32_t> ident(waves / 4);
    for (size_t i = 0; i < ident.size(); ++i) ident[i] = (uint32_t)i;
    if (int rc = c->order.alloc(c, ident.size())) return rc;
    VX_HIP(c, hipMemcpy(c->order, ident.data(), ident.size() * 4, hipMemcpyHostToDevice));
    c->order_builds_left = 2;
    c->miss.split_stale = true;
  }
  return VX_OK;
}

// ---- shadowed DVR: the light grid (vx_shadow.hpp) ---------------------------------------------------
static bool shadow_on(const VxContext* c) {
  const VxParams& p = c->params;
  return p.render_mode == VX_MODE_DVR && p.dvr_shadow_stride != 0 && !p.debug_hits;
}
// the light march of every node, with fp32 operations a NumPy restatement repeats (tests/shadow_ref.py)
static LightMarch light_march(const VxContext* c) {
  const VxParams& p = c->params;
  const float* m = p.density_transform_inv;
  LightMarch lm{};
  const float lx = -p.light_dir[0], ly = -p.light_dir[1], lz = -p.light_dir[2];
  for (int i = 0; i < 3; ++i) lm.idir[i] = fmaf(m[8 + i], lz, fmaf(m[4 + i], ly, m[i] * lx));   // mat3(dti) * (-light_dir)
  lm.dt = p.dvr_step_voxels / sqrtf(fmaf(lm.idir[2], lm.idir[2], fmaf(lm.idir[1], lm.idir[1], lm.idir[0] * lm.idir[0])));
  // the clip box in index space: the bounds of its eight corners mapped as prepare_render maps them
  for (int i = 0; i < 3; ++i) {
    lm.box_lo[i] = INFINITY;
    lm.box_hi[i] = -INFINITY;
  }
  for (int corner = 0; corner < 8; ++corner) {
    const float w[3] = {(corner & 1) ? p.volume_aabb_max[0] : p.volume_aabb_min[0],
                        (corner & 2) ? p.volume_aabb_max[1] : p.volume_aabb_min[1],
                        (corner & 4) ? p.volume_aabb_max[2] : p.volume_aabb_min[2]};
    for (int i = 0; i < 3; ++i) {
      const float q = fmaf(m[12 + i], 1.0f, fmaf(m[8 + i], w[2], fmaf(m[4 + i], w[1], m[i] * w[0])));
      lm.box_lo[i] = std::min(lm.box_lo[i], q);
      lm.box_hi[i] = std::max(lm.box_hi[i], q);
    }
  }
  const uint32_t s = (uint32_t)p.dvr_shadow_stride;
  lm.stride = s;
  for (int i = 0; i < 3; ++i) {
    lm.n[i] = (c->vol.dv.extent[i] - 1u + s - 1u) / s + 1u;   // ceil((extent - 1) / s) + 1
    // nodes inside the box: box_lo <= s * i + 1/2 <= box_hi (prepare_render keeps the box within the volume)
    const double lo = std::ceil(((double)lm.box_lo[i] - 0.5) / s), hi = std::floor(((double)lm.box_hi[i] - 0.5) / s);
    lm.ilo[i] = (uint32_t)std::min(std::max(lo, 0.0), (double)(lm.n[i] - 1u));
    lm.ihi[i] = (uint32_t)std::min(std::max(hi, (double)lm.ilo[i]), (double)(lm.n[i] - 1u));
  }
  return lm;
}
// build the light grid on the context's stream (after the layouts of the launch are in place)
static int rebuild_light_grid(VxContext* c) {
  c->vol.shadow_table.stale = true;   // until this build is complete
  const LightMarch lm = light_march(c);
  const uint64_t nodes = (uint64_t)lm.n[0] * lm.n[1] * lm.n[2];
  if (nodes >= (1ull << 31))
    VX_FAIL(c, VX_ERR_INVALID, "shadowed DVR: a light grid of %llu nodes (stride %u) is beyond the look-up's index range; "
            "use a larger dvr_shadow_stride", (unsigned long long)nodes, lm.stride);
  if (nodes > c->vol.shadow_dev.cap) {
    VX_HIP(c, hipStreamSynchronize(c->stream));   // no queued launch still reads the old grid
    c->vol.shadow = ShadowGrid{};
    if (int rc = c->vol.shadow_dev.alloc(c, nodes)) return rc;
  }
  if (int rc = c->shadow_count_dev.ensure(c, 1)) return rc;
  VX_HIP(c, hipMemsetAsync(c->shadow_count_dev, 0, sizeof(unsigned long long), c->stream));
  const dim3 grid((lm.n[0] + 7u) / 8u, (lm.n[1] + 7u) / 8u, (lm.n[2] + 3u) / 4u);
  const size_t lds = c->tf_len <= TF_LDS_MAX ? (size_t)c->tf_len * sizeof(float4) : 0u;
  if (int rc = c->shadow_timer.mark(c, 0)) return rc;
  with_layout(eff_layout(c), [&](auto tag) {
    constexpr int LAY = decltype(tag)::value;
    hipLaunchKernelGGL((build_light_grid<LAY>), grid, dim3(256), lds, c->stream, c->params, c->vol.dv, c->tf, c->tf_len, lm,
                       c->vol.shadow_dev, c->shadow_count_dev);
  });
  VX_HIP(c, hipGetLastError());
  if (int rc = c->shadow_timer.mark(c, 1)) return rc;
  ShadowGrid& g = c->vol.shadow;
  g.t = c->vol.shadow_dev;
  g.inv_s = 1.0f / (float)lm.stride;
  for (int i = 0; i < 3; ++i) {
    g.n[i] = lm.n[i];
    g.glo[i] = (float)lm.ilo[i];
    g.ghi[i] = (float)lm.ihi[i];
    g.gmax[i] = (float)(lm.n[i] - 1u);
  }
  c->vol.shadow_table.built(c->params);
  c->shadow_builds += 1;
  return VX_OK;
}

// the blocks of one frame slot of a render launch: 16 per 64x64 tile of the shard (4 waves of 8x8 pixels each), the tiles in
// groups of 8
static uint32_t frame_blocks(const VxContext* c) { return (c->tm.tiles_per_shard + 7u) / 8u * 128u; }

// ---- the launch plan: the kernel instance a render launch runs, its launch shape, and whether it folds the running mean ---

enum class Kernel {
  DVR_LDS,    // LDS-window DVR / Phong: render_dvr_lds, render_dvr_lds_shadow (vx_dvr_lds.hpp)
  PROJ_LDS,   // LDS-window intensity projections: render_proj_lds (vx_projection.hpp)
  DVR_CQ,     // tuned DVR on the cellquad layout: render_dvr_cq (vx_dvr.hpp)
  GENERIC,    // render_generic<MODE, LAYOUT>, render_generic_shadow (vx_kernels.hpp, vx_shadow.hpp)
};
// Everything a render launch needs besides the frame slots and the weight: the instance (kernel family and template
// arguments), the launch shape, and the kernel's extra argument.
struct LaunchPlan {
  Kernel kernel = Kernel::GENERIC;
  int mode = VX_MODE_DVR;             // render_generic's MODE
  int layout = VX_LAYOUT_REFERENCE;   // render_generic's LAYOUT (with_layout); the tuned kernels are each for one layout
  bool phong = false;                 // DVR_LDS: PHONG
  bool minip = false;                 // PROJ_LDS: MINIP
  bool shadow = false;                // DVR_LDS, GENERIC: the shadowed kernel, with `light` as its extra argument
  bool skip = false;                  // DVR_LDS, DVR_CQ: SKIP (the macro-cell mask); PROJ_LDS: SKIP, with `bounds`
  bool u8 = false;                    // DVR_LDS, PROJ_LDS: U8 (staged from the bricku8 layout)
  bool probe = false;                 // DVR_CQ: PROBE (vx_probe_gather_spread's measurement build)
  ShadowGrid light{};                 // the light grid of a shadowed launch
  const float* bounds = nullptr;      // PROJ_LDS: the table of range skipping, nullptr without SKIP
  const uint32_t* order = nullptr;    // the tuned kernels' block order, longest first (build_order); nullptr: the probe's
  dim3 grid, block{256};
  // DVR_LDS, a split launch (VxContext::MissSplit): `grid` and `order` cover the blocks that may hit the clip box, and
  // render_dvr_miss runs the rest -- miss_grid.x launch slots (0: no split) in the order miss_order; one logical launch
  dim3 miss_grid{0};
  const uint32_t* miss_order = nullptr;
  size_t lds = 0;                     // dynamic LDS bytes
  bool fuse = false;                  // the kernel folds the running mean of the launch itself (MultiOut::fuse)
  bool segv = false;                  // DVR_LDS, PROJ_LDS: the segment view's kernel (render_dvr_lds_seg, render_proj_lds_seg)
  const uint32_t* segm = nullptr;     // its segment mask (SegDev::seg as dwords)
  uint32_t seg_inv = 0u;              // 0: ONLY, ~0u: HIDE
};

static bool tuned_possible(const VxContext* c) {
  // (an early-termination threshold <= 0 -- an epsilon >= 1: every ray ends at its first contributing sample -- is
  // served by render_generic, whose Frame::dvr spells the test as the oracle does; the tuned kernels assume tau >= ert
  // implies a contributing sample)
  // (the projections have no early termination: dvr_ert_tau does not matter to them)
  return c->sw.dvr_variant != 0 && !c->params.debug_hits && c->tf_len <= TF_LDS_MAX &&
         (c->params.dvr_ert_tau > 0.0f || proj_mode(c->params.render_mode));
}
// the LDS-window kernel (vx_dvr_lds.hpp): DVR on the brickf32 layout, Phong wherever brickf32 data is resident; the
// projections' form of it (vx_projection.hpp) on brickf32 and bricku8
static bool use_lds_kernel(const VxContext* c) {
  if (!tuned_possible(c)) return false;
  if (proj_mode(c->params.render_mode))
    return eff_layout(c) == VX_LAYOUT_BRICKF32 || (eff_layout(c) == VX_LAYOUT_BRICKU8 && c->vol.dv.bu != nullptr);
  if (eff_layout(c) == VX_LAYOUT_BRICKU8)   // the same kernel, staging from the 8-bit bricks
    return (c->params.render_mode == VX_MODE_DVR || c->params.render_mode == VX_MODE_DVR_PHONG) && c->vol.dv.bu != nullptr;
  if (c->params.render_mode == VX_MODE_DVR) return eff_layout(c) == VX_LAYOUT_BRICKF32;
  return c->params.render_mode == VX_MODE_DVR_PHONG && c->vol.dv.bf != nullptr;
}
static bool is_tuned(const VxContext* c) {
  const bool dvr_cq = c->params.render_mode == VX_MODE_DVR && eff_layout(c) == VX_LAYOUT_CELLQUAD;
  return tuned_possible(c) && (dvr_cq || use_lds_kernel(c));
}
// The fuse rule: whether `kernel` folds the running mean of an n-frame launch of render mode `mode` itself -- the LDS-window
// kernels at 8, 16, 32 or 64 frames (a wave holds every frame of its 8, 4, 2 or 1 pixels), render_generic for `default`,
// `no_dda` or `raymarch` at exactly 32 frames (2 pixels x 32 frames per wave).  Every other multi-frame launch writes
// per-frame result slabs that merge_results blends in frame order.
static bool lds_window_kernel(Kernel k) { return k == Kernel::DVR_LDS || k == Kernel::PROJ_LDS; }
static bool folds(Kernel kernel, int mode, uint32_t n) {
  switch (kernel) {
    case Kernel::DVR_LDS:
    case Kernel::PROJ_LDS: return n == 8u || n == 16u || n == 32u || n == 64u;
    case Kernel::GENERIC: return mode <= VX_MODE_RAYMARCH && n == 32u;
    default: return false;
  }
}
// the dynamic LDS of a launch: the TF, the mask of the empty-space grid where the kernel stages it, the wave tiles
static size_t lds_bytes(const VxContext* c, const LaunchPlan& lp) {
  const size_t tf = (size_t)c->tf_len * sizeof(float4);
  const size_t mask = lp.skip ? (size_t)c->vol.dv.skip_words * 4u : 0u;
  const size_t tiles = 4u * (size_t)(lp.phong ? LdsTile<true>::FLOATS : LdsTile<false>::FLOATS) * sizeof(float);
  switch (lp.kernel) {
    case Kernel::DVR_LDS: return tf + ((mask + 15u) & ~(size_t)15u) + tiles;   // the mask in whole 16-byte rows
    case Kernel::PROJ_LDS: return tf + tiles;                                   // the bounds stay in global memory
    case Kernel::DVR_CQ: return tf + mask;
    default: return (c->tf_len <= TF_LDS_MAX ? tf : 0u) + (lp.fuse ? 4u * 320u * sizeof(float) : 0u);   // + fold_frames' scratch
  }
}
// The one place that decides what a render launch of the mo.count frame slots of `mo` runs (after prepare_render).  The
// kernel folds the running mean of the launch itself while VX_DVR_FUSE is on and the fuse rule (folds) says it does.
static LaunchPlan plan_launch(const VxContext* c, const MultiOut& mo, bool probe = false) {
  const VxParams& p = c->params;
  LaunchPlan lp;
  lp.mode = p.render_mode;
  lp.layout = eff_layout(c);
  lp.shadow = shadow_on(c);
  // shadowed DVR: the LDS-window kernel's shadowed form, or render_generic's -- never the cellquad DVR kernel
  if (is_tuned(c) && (!lp.shadow || use_lds_kernel(c)))
    lp.kernel = !use_lds_kernel(c) ? Kernel::DVR_CQ : proj_mode(p.render_mode) ? Kernel::PROJ_LDS : Kernel::DVR_LDS;
  lp.phong = lp.kernel == Kernel::DVR_LDS && p.render_mode == VX_MODE_DVR_PHONG;
  lp.minip = lp.kernel == Kernel::PROJ_LDS && p.render_mode == VX_MODE_MINIP;
  if (lp.shadow) lp.light = c->vol.shadow;
  // SKIP: the DVR kernels test that a mask exists, the projections that their bounds are current
  if (lp.kernel == Kernel::PROJ_LDS) {
    lp.skip = p.dvr_skip_empty && c->proj_dev && !c->vol.proj_table.stale;
    lp.bounds = lp.skip ? c->proj_dev : nullptr;
  } else {
    lp.skip = p.dvr_skip_empty && c->vol.dv.skip_bits;
  }
  // the segment view (check_segment_view has refused every launch it does not cover): the masked instance, without skipping
  if (c->vol.seg_view != VX_SEGVIEW_OFF && lds_window_kernel(lp.kernel)) {
    lp.segv = true;
    lp.segm = reinterpret_cast<const uint32_t*>(c->vol.seg.seg);
    lp.seg_inv = c->vol.seg_view == VX_SEGVIEW_HIDE ? ~0u : 0u;
    lp.skip = false;
    lp.bounds = nullptr;
  }
  lp.u8 = lp.layout == VX_LAYOUT_BRICKU8 && c->vol.dv.bu;
  lp.probe = probe;
  lp.order = probe ? nullptr : c->order;
  // a frame's blocks per frame slot (the LDS-window kernels take a count of 0 as 1)
  const bool lds_window = lds_window_kernel(lp.kernel);
  lp.grid = dim3(frame_blocks(c) * (lds_window && mo.count == 0u ? 1u : mo.count));
  lp.fuse = c->sw.dvr_fuse && folds(lp.kernel, lp.mode, mo.count);
  lp.lds = lds_bytes(c, lp);
  // the split: a multi-frame launch of plain DVR on the LDS-window kernel, with a proof for some block and both halves of
  // the order in place.  Not a single-frame launch: it is bound by the latency of its longest rays, the missing waves ran
  // beside them for nothing, and split it measured 5 % slower (NOTEBOOK R4.13).
  const VxContext::MissSplit& ms = c->miss;
  if (lp.kernel == Kernel::DVR_LDS && !lp.phong && !lp.shadow && !lp.segv && mo.count > 1u && c->sw.dvr_miss && ms.proved > 0u &&
      ms.table.current(p) && ms.blocks == frame_blocks(c) && !ms.split_stale) {
    lp.grid = dim3((ms.blocks - ms.n_miss) * mo.count);
    lp.order = ms.order_heavy;
    lp.miss_grid = dim3(ms.n_miss * mo.count);
    lp.miss_order = ms.order_miss;
  }
  return lp;
}

// calls f(std::integral_constant<int, VX_MODE_*>) for render mode m
template <class F>
static void with_mode(int m, F&& f) {
  switch (m) {
    case VX_MODE_DEFAULT: f(std::integral_constant<int, VX_MODE_DEFAULT>{}); break;
    case VX_MODE_NO_DDA: f(std::integral_constant<int, VX_MODE_NO_DDA>{}); break;
    case VX_MODE_RAYMARCH: f(std::integral_constant<int, VX_MODE_RAYMARCH>{}); break;
    case VX_MODE_DVR: f(std::integral_constant<int, VX_MODE_DVR>{}); break;
    case VX_MODE_MIP: f(std::integral_constant<int, VX_MODE_MIP>{}); break;
    case VX_MODE_MINIP: f(std::integral_constant<int, VX_MODE_MINIP>{}); break;
    default: f(std::integral_constant<int, VX_MODE_DVR_PHONG>{}); break;
  }
}

// The one launch switch: runs the instance `lp` names for the frame slots of `mo` on the context's stream.  Fails closed: a
// launch with mo.fuse set that the fuse rule does not fold is refused -- its frames would reach no accumulator.
static int launch_planned(VxContext* c, const LaunchPlan& lp, const MultiOut& mo, float weight) {
  if (mo.fuse && !folds(lp.kernel, lp.mode, mo.count))
    VX_FAIL(c, VX_ERR_INVALID, "render launch: running mean to fold (MultiOut::fuse) for a kernel that does not fold it");
  const VxParams& p = c->params;
  const DevVolume& v = c->vol.dv;
  const TileMap& tm = c->tm;
  const float4* tf = c->tf;
  const uint32_t n = c->tf_len;
  const hipStream_t s = c->stream;
  switch (lp.kernel) {
    case Kernel::DVR_LDS:
      if (lp.segv) {
        with_bool(lp.u8, [&](auto u8) {
          with_bool(lp.phong, [&](auto ph) {
            constexpr bool PH = decltype(ph)::value;
            hipLaunchKernelGGL((render_dvr_lds_seg<(PH ? VX_LDS_S_PHONG : VX_LDS_S), PH, decltype(u8)::value>), lp.grid, lp.block,
                               lp.lds, s, p, v, tf, n, mo, weight, tm, lp.order, lp.segm, lp.seg_inv);
          });
        });
        break;
      }
      if (lp.miss_grid.x != 0u)   // the blocks that cannot hit the clip box: the same frame slots, the same fold
        hipLaunchKernelGGL(render_dvr_miss, lp.miss_grid, lp.block, mo.fuse ? 4u * 320u * sizeof(float) : 0u, s, p, v, tf, n, mo,
                           weight, tm, lp.miss_order);   // (LDS: fold_frames' scratch, 320 floats per wave, in a launch that folds)
      if (lp.grid.x == 0u) break;   // (no block of this shard can hit)
      with_bool(lp.skip, [&](auto sk) {
        with_bool(lp.u8, [&](auto u8) {
          constexpr bool SK = decltype(sk)::value, U8 = decltype(u8)::value;
          if (lp.shadow) {   // (vx_set_params refuses a stride with Phong)
            hipLaunchKernelGGL((render_dvr_lds_shadow<VX_LDS_S, SK, U8>), lp.grid, lp.block, lp.lds, s, p, v, tf, n, mo, weight, tm,
                               lp.order, lp.light);
            return;
          }
          with_bool(lp.phong, [&](auto ph) {
            constexpr bool PH = decltype(ph)::value;
            hipLaunchKernelGGL((render_dvr_lds<(PH ? VX_LDS_S_PHONG : VX_LDS_S), PH, SK, U8>), lp.grid, lp.block, lp.lds, s, p, v, tf,
                               n, mo, weight, tm, lp.order);
          });
        });
      });
      break;
    case Kernel::PROJ_LDS:
      if (lp.segv) {
        with_bool(lp.minip, [&](auto mi) {
          with_bool(lp.u8, [&](auto u8) {
            hipLaunchKernelGGL((render_proj_lds_seg<VX_LDS_S, decltype(mi)::value, decltype(u8)::value>), lp.grid, lp.block, lp.lds, s,
                               p, v, tf, n, mo, weight, tm, lp.order, lp.segm, lp.seg_inv);
          });
        });
        break;
      }
      with_bool(lp.minip, [&](auto mi) {
        with_bool(lp.skip, [&](auto sk) {
          with_bool(lp.u8, [&](auto u8) {
            hipLaunchKernelGGL((render_proj_lds<VX_LDS_S, decltype(mi)::value, decltype(sk)::value, decltype(u8)::value>), lp.grid,
                               lp.block, lp.lds, s, p, v, tf, n, mo, weight, tm, lp.order, lp.bounds);
          });
        });
      });
      break;
    case Kernel::DVR_CQ:   // 4 march steps per batch
      with_bool(lp.skip, [&](auto sk) {
        with_bool(lp.probe, [&](auto pr) {
          hipLaunchKernelGGL((render_dvr_cq<4, decltype(sk)::value, decltype(pr)::value>), lp.grid, lp.block, lp.lds, s, p, v, tf, n,
                             mo, weight, tm, lp.order);
        });
      });
      break;
    default:
      with_layout(lp.layout, [&](auto lay) {
        constexpr int LAY = decltype(lay)::value;
        if (lp.shadow) {
          hipLaunchKernelGGL((render_generic_shadow<LAY>), lp.grid, lp.block, lp.lds, s, p, v, tf, n, mo, weight, tm, lp.light);
          return;
        }
        with_mode(lp.mode, [&](auto m) {
          hipLaunchKernelGGL((render_generic<decltype(m)::value, LAY>), lp.grid, lp.block, lp.lds, s, p, v, tf, n, mo, weight, tm);
        });
      });
  }
  VX_HIP(c, hipGetLastError());
  {
    const uint32_t slots = mo.count == 0u ? 1u : mo.count;
    c->miss.last_heavy = lp.grid.x / slots;
    c->miss.last_miss = lp.miss_grid.x / slots;
  }
  return VX_OK;
}

// point the detile kernel's table at these slabs (entries in stream order: rewritten only when they change)
static int set_slab_table(VxContext* c, const std::vector<const float4*>& t) {
  if (t == c->slab_table_host) return VX_OK;
  c->slab_table_host.clear();
  VX_HIP(c, hipStreamSynchronize(c->stream));   // no queued de-tile still reads the old table
  if (int rc = c->slab_table.ensure(c, t.size())) return rc;
  VX_HIP(c, hipMemcpy(c->slab_table, t.data(), t.size() * sizeof(float4*), hipMemcpyHostToDevice));
  c->slab_table_host = t;
  return VX_OK;
}

// the slabs of the table -> row-major image (W x H float4) on the context's stream
static int launch_detile(VxContext* c, float4* image) {
  if (c->slab_table_host.size() != c->tm.shard_count)
    VX_FAIL(c, VX_ERR_INVALID, "detile: %zu slabs for %u shards", c->slab_table_host.size(), c->tm.shard_count);
  dim3 grid((c->W + 15) / 16, (c->H + 15) / 16);
  hipLaunchKernelGGL(detile, grid, dim3(256), 0, c->stream, (const float4* const*)c->slab_table, image, c->tm);
  VX_HIP(c, hipGetLastError());
  return VX_OK;
}

// The row-major image the vx_read_* calls read, de-tiled into the image of the context returned through d.  A plain
// context: its own slab, the tiles of other shards reading as zero.  A group: every member's slab read in place by one
// de-tile on the display device (member 0), whose stream first waits for each member's last render.
static int compose_image(VxContext* c, VxContext*& d) {
  if (!is_group(c)) {
    d = c;
    if (!c->slab) VX_FAIL(c, VX_ERR_INVALID, "no framebuffer (vx_resize not called)");
    std::vector<const float4*> t(c->tm.shard_count, nullptr);
    t[c->tm.shard_rank] = c->slab;
    int rc = set_slab_table(c, t);
    return rc ? rc : launch_detile(c, c->image);
  }
  d = c->members[0];
  if (!d->has_params) VX_FAIL(c, VX_ERR_INVALID, "a device group is read after vx_set_params (which deals the shards)");
  std::vector<const float4*> t(c->members.size());
  for (size_t i = 0; i < t.size(); ++i) {
    VxContext* m = c->members[i];
    if (!m->slab) VX_FAIL(c, VX_ERR_INVALID, "member %zu (device %d): no framebuffer (vx_resize not called)", i, m->device);
    if (m->W != d->W || m->H != d->H || m->tm.shard_count != t.size())
      VX_FAIL(c, VX_ERR_INVALID, "member %zu (device %d): framebuffer differs from member 0's", i, m->device);
    t[i] = m->slab;
  }
  VX_HIP(c, hipSetDevice(d->device));
  if (int rc = set_slab_table(d, t)) return member_fail(c, 0, rc);
  for (size_t i = 1; i < t.size(); ++i) {
    VxContext* m = c->members[i];
    VX_HIP(c, hipSetDevice(m->device));
    VX_HIP(c, hipEventRecord(m->done, m->stream));
  }
  VX_HIP(c, hipSetDevice(d->device));
  for (size_t i = 1; i < t.size(); ++i) VX_HIP(c, hipStreamWaitEvent(d->stream, c->members[i]->done, 0));
  return on_member0(c, launch_detile(d, d->image));
}

// The split of a plain multi-frame DVR launch of the LDS-window kernel, kept current the way the derived tables are: the
// classification is rebuilt when the bits of its key change or the tile map did, the two halves of the block order when `order`
// or the flags did.  Called at the end of prepare_render ahead of a multi-frame launch only (the counters and `order` exist):
// single-frame launches are never split (NOTEBOOK R4.13) and pay nothing for it.  plan_launch uses what it finds current.
static int ensure_miss_split(VxContext* c) {
  VxContext::MissSplit& ms = c->miss;
  const VxParams& p = c->params;
  if (!c->sw.dvr_miss || p.render_mode != VX_MODE_DVR || !use_lds_kernel(c)) return VX_OK;
  const uint32_t nb = frame_blocks(c);
  if (!ms.table.current(p) || ms.blocks != nb) {
    ms.table.stale = true;   // until this build is complete: a failure below must not leave the old key over new counts
    std::vector<uint8_t> img;
    ms.proved = ms.n_miss = 0;
    ms.blocks = nb;
    if (classify_miss_blocks(p, c->W, c->H, img) != 0u) {
      // image block -> logical block of this shard: block_to_tile, tile_at and wave_pixel on the host
      const TileMap& tm = c->tm;
      const uint32_t nbx = (c->W + 15u) / 16u;
      auto morton_x = [](uint32_t m) { return (m & 1u) | ((m >> 1) & 2u) | ((m >> 2) & 4u); };
      ms.flags_host.assign(nb, 0);
      for (uint32_t b = 0; b < nb; ++b) {
        const uint32_t lt = (b >> 7) * 8u + (b & 7u), wt = ((b >> 3) & 15u) * 4u;
        const uint32_t pos = lt * tm.shard_count + tm.shard_rank;
        const uint32_t t = (!c->tile_perm_host.empty() && pos < tm.n_tiles) ? c->tile_perm_host[pos] : pos;
        const uint32_t x0 = (t % tm.tiles_x) * 64u + morton_x(wt) * 8u, y0 = (t / tm.tiles_x) * 64u + morton_x(wt >> 1) * 8u;
        if (lt >= tm.tiles_per_shard || t >= tm.n_tiles || x0 >= tm.W || y0 >= tm.H) {
          ms.flags_host[b] = 1;   // no pixel: either kernel returns at once
        } else if (img[(size_t)(y0 >> 4) * nbx + (x0 >> 4)]) {
          ms.flags_host[b] = 1;
          ms.proved += 1;
        }
        ms.n_miss += ms.flags_host[b];
      }
    }
    if (ms.proved > 0u) {
      if (ms.flags.cap < nb || ms.order_heavy.cap < nb || ms.order_miss.cap < nb) {
        VX_HIP(c, hipStreamSynchronize(c->stream));   // no queued launch still reads the old halves
        if (int rc = ms.flags.alloc(c, nb)) return rc;
        if (int rc = ms.order_heavy.alloc(c, nb)) return rc;
        if (int rc = ms.order_miss.alloc(c, nb)) return rc;
      }
      VxContext::MissSplit::Stage& st = ms.stage[ms.next_stage];
      ms.next_stage ^= 1;
      if (st.pending) VX_HIP(c, hipEventSynchronize(st.done));
      st.pending = false;
      if (st.cap < nb) {
        if (st.p) (void)hipHostFree(st.p);
        st.p = nullptr;
        st.cap = 0;
        VX_HIP(c, hipHostMalloc(reinterpret_cast<void**>(&st.p), nb, hipHostMallocDefault));
        st.cap = nb;
      }
      if (!st.done) VX_HIP(c, hipEventCreateWithFlags(&st.done, hipEventDisableTiming));
      memcpy(st.p, ms.flags_host.data(), nb);
      VX_HIP(c, hipMemcpyAsync(ms.flags, st.p, nb, hipMemcpyHostToDevice, c->stream));
      VX_HIP(c, hipEventRecord(st.done, c->stream));
      st.pending = true;
    }
    ms.table.built(p);
    ms.split_stale = true;
  }
  if (ms.proved > 0u && ms.split_stale) {
    hipLaunchKernelGGL(split_order, dim3(1), dim3(1024), 0, c->stream, c->order, ms.flags, nb, ms.order_heavy, ms.order_miss);
    VX_HIP(c, hipGetLastError());
    ms.split_stale = false;
  }
  return VX_OK;
}

// multi: a multi-frame launch follows (vx_render_frames)
static int prepare_render(VxContext* c, bool multi = false) {
  if (!c->vol.has_volume) VX_FAIL(c, VX_ERR_NO_VOLUME, "vx_render_frame: no volume uploaded");
  if (!c->has_params) VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: vx_set_params not called");
  if (!c->tf) VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: no transfer function");
  if (!c->slab) VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: vx_resize not called");
  if ((uint32_t)c->params.res[0] != c->W || (uint32_t)c->params.res[1] != c->H)
    VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: params.res differs from the framebuffer size");
  if (c->params.use_env > 0 && !c->env_tex)
    VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: use_env = 1 without vx_upload_environment");
  c->vol.dv.env_tex = c->env_tex;
  c->vol.dv.env_imp = c->env_imp;
  c->vol.dv.env_impq = c->env_impq;
  c->vol.dv.env_avg_w = c->env_avg_w;
  c->vol.dv.env_w = c->env_w;
  c->vol.dv.env_h = c->env_h;
  {
    // The box the rays are clipped to must lie inside the volume (volume.ts:32-37 clips the volume's own box, so the
    // viewer cannot ask for anything else): the trilinear look-up of the cellquad layout relies on every sample's cell
    // lying in the apron lattice (Frame::trilinear, IN_LATTICE), i.e. on index positions within [-1/2, extent + 1/2).
    // A quarter voxel of that margin is left to the rounding of ray positions near the faces.
    const VxParams& p = c->params;
    for (int corner = 0; corner < 8; ++corner) {
      const float w[3] = {(corner & 1) ? p.volume_aabb_max[0] : p.volume_aabb_min[0],
                          (corner & 2) ? p.volume_aabb_max[1] : p.volume_aabb_min[1],
                          (corner & 4) ? p.volume_aabb_max[2] : p.volume_aabb_min[2]};
      for (int i = 0; i < 3; ++i) {
        const float* m = p.density_transform_inv;
        const float q = fmaf(m[12 + i], 1.0f, fmaf(m[8 + i], w[2], fmaf(m[4 + i], w[1], m[i] * w[0])));
        if (!(q >= -0.25f && q <= (float)c->vol.dv.extent[i] + 0.25f))
          VX_FAIL(c, VX_ERR_INVALID, "vx_render_frame: volume_aabb reaches index %.3f on axis %d, outside the volume [0, %u]: "
                  "the clip box must lie inside the volume's own box (volume.ts:32-37)", (double)q, i, c->vol.dv.extent[i]);
      }
    }
  }
  {
    // the wave-uniform terms of the primary ray (DevVolume::cam_o ...), with the operations of setup_world_ray /
    // to_index (vx_device.hpp): fma chains in the same order, IEEE divisions -- the same bits as on the device
    const VxParams& p = c->params;
    auto mat4 = [](const float* m, float x, float y, float z, float w, float out[4]) {
      for (int i = 0; i < 4; ++i) out[i] = fmaf(m[12 + i], w, fmaf(m[8 + i], z, fmaf(m[4 + i], y, m[i] * x)));
    };
    float cw[4], a[4];
    mat4(p.camera_view_inv, 0.0f, 0.0f, 0.0f, 1.0f, cw);
    for (int i = 0; i < 3; ++i) c->vol.dv.cam_o[i] = cw[i] / cw[3];
    mat4(p.density_transform_inv, c->vol.dv.cam_o[0], c->vol.dv.cam_o[1], c->vol.dv.cam_o[2], 1.0f, a);
    for (int i = 0; i < 3; ++i) c->vol.dv.cam_ipos[i] = a[i];
    c->vol.dv.inv_res[0] = 1.0f / (float)p.res[0];
    c->vol.dv.inv_res[1] = 1.0f / (float)p.res[1];
    // the per-ray divisions a launch constant decides (DevVolume::ray_flags): both shortcuts are exact or not taken
    uint32_t flags = 0;
    const float* vi = p.camera_view_inv;
    if (vi[3] == 0.0f && vi[7] == 0.0f && vi[11] == 0.0f && vi[15] == 1.0f) flags |= RAY_AFFINE_VIEW;
    for (int axis = 0; axis < 2; ++axis) {
      if (c->tex_checked_res[axis] != p.res[axis]) {   // tried once per resolution, not per launch
        const float res = (float)p.res[axis], y = c->vol.dv.inv_res[axis];
        bool same = true;
        for (int px = 0; px < p.res[axis] && same; ++px) {
          const float a = (float)px + 0.5f, q0 = a * y;
          same = fmaf(fmaf(-res, q0, a), y, q0) == a / res;
        }
        c->tex_checked_res[axis] = p.res[axis];
        c->tex_by_reciprocal[axis] = same;
      }
      if (c->tex_by_reciprocal[axis]) flags |= (axis == 0 ? RAY_TEX_BY_RECIPROCAL_X : RAY_TEX_BY_RECIPROCAL_Y);
    }
    if (!c->sw.ray_shortcuts) flags = 0;   // diagnostic: the divisions themselves
    c->vol.dv.ray_flags = flags;
  }
  {
    const VxParams& p = c->params;
    const bool dvr = p.render_mode == VX_MODE_DVR || p.render_mode == VX_MODE_DVR_PHONG;
    int rc = VX_OK;
    if (dvr && p.dvr_skip_empty && !p.debug_hits && !c->vol.skip_table.current(p)) rc = rebuild_skip_mask(c);
    if (!rc && proj_mode(p.render_mode) && p.dvr_skip_empty && !p.debug_hits && !c->vol.proj_table.current(p))
      rc = rebuild_projection_bounds(c);
    if (!rc && p.render_mode == VX_MODE_DEFAULT && !p.debug_hits && !c->vol.lmaj_table.current(p)) rc = rebuild_local_majorants(c);
    if (rc) return rc;
  }
  {
    // the layouts this launch samples, made resident on first use beside the one the upload built; dvr_phong runs on the
    // LDS-window kernel, which samples brickf32: a context on cellquad gets the bricks beside it the first time Phong is rendered
    int lay = eff_layout(c);
    int rc = VX_OK;
    if (lay == VX_LAYOUT_CELLQUAD) {
      rc = ensure_layout(c, VX_LAYOUT_CELLQUAD);
      lay = eff_layout(c);   // AUTO may have stepped down to the resident bricks (memory budget)
    }
    if (!rc && (lay == VX_LAYOUT_BRICKF32 ||
                (c->params.render_mode == VX_MODE_DVR_PHONG && lay == VX_LAYOUT_CELLQUAD && tuned_possible(c))))
      rc = ensure_layout(c, VX_LAYOUT_BRICKF32);
    if (rc) return rc;
  }
  if (int rc = check_segment_view(c, "vx_render_frame", false)) return rc;
  if (shadow_on(c) && !c->vol.shadow_table.current(c->params)) {   // after the layouts: the build samples them
    int rc = rebuild_light_grid(c);
    if (rc) return rc;
  }
  if (int rc = ensure_counters(c, (size_t)frame_blocks(c) * 4u)) return rc;  // one record per wave of a frame's blocks
  return multi ? ensure_miss_split(c) : VX_OK;
}

static int take_events(VxContext* c, EventPair& ev) {
  if (c->free_events.empty()) {
    if (c->pending_events.size() >= 4096) drain_events(c);
    if (c->free_events.empty()) {
      VX_HIP(c, hipEventCreate(&ev.a));
      VX_HIP(c, hipEventCreate(&ev.b));
      return VX_OK;
    }
  }
  ev = c->free_events.back();
  c->free_events.pop_back();
  return VX_OK;
}

// at least n slots of per-frame result slabs and counter records for the current framebuffer and grid (grow-only)
static int ensure_pipes(VxContext* c, uint32_t n) {
  if (c->pipe_slots >= n && c->pipe_quads == c->slab_quads && c->pipe_waves == c->dc_waves) return VX_OK;
  VX_HIP(c, hipStreamSynchronize(c->stream));
  {
    int rc = fold_counters(c);   // keep what the records of the old slots have counted
    if (rc) return rc;
  }
  const size_t ns = std::max(n, c->pipe_slots), waves = c->dc_waves;
  c->pipe_result_pool.reset();
  c->pipe_dc_pool.reset();
  c->pipe_slots = 0;
  if (int rc = c->pipe_result_pool.alloc(c, ns * c->slab_quads)) return rc;
  if (int rc = c->pipe_dc_pool.alloc(c, ns * waves)) return rc;
  VX_HIP(c, hipMemsetAsync(c->pipe_dc_pool, 0, ns * waves * sizeof(DevCounters), c->stream));   // ordered with the launches
  VX_HIP(c, hipStreamSynchronize(c->stream));
  c->pipe_slots = (uint32_t)ns;
  c->pipe_quads = c->slab_quads;
  c->pipe_waves = waves;
  return VX_OK;
}

}  // namespace

// The segment view's refusals, in one place: a covered call (`iso`: vx_isosurface; else a render launch, after its layouts are
// resident) with the view on fails here, before anything is launched, unless a masked instance serves it.
int vx::check_segment_view(VxContext* c, const char* fn, bool iso) {
  if (c->vol.seg_view == VX_SEGVIEW_OFF) return VX_OK;
  const char* view = c->vol.seg_view == VX_SEGVIEW_ONLY ? "only" : "hide";
  if (is_group(c)) VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s: not for a device group (the segment lives on member 0)", fn, view);
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s without a current segment (vx_segment first; an upload drops it)", fn, view);
  if (iso) return VX_OK;
  const VxParams& p = c->params;
  if (p.render_mode <= VX_MODE_RAYMARCH)
    VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s: not for the path-traced render mode %d (default, no_dda, raymarch)", fn, view,
            p.render_mode);
  if (p.debug_hits) VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s: not with debug_hits", fn, view);
  if (p.dvr_shadow_stride != 0)
    VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s: not for shadowed DVR (dvr_shadow_stride = %d)", fn, view, p.dvr_shadow_stride);
  if (!use_lds_kernel(c))
    VX_FAIL(c, VX_ERR_INVALID, "%s: segment view %s: this launch has no LDS-window kernel (layout %d, dvr_ert_tau <= 0, a TF of "
            "more than %u entries or VX_DVR_KERNEL=generic)", fn, view, eff_layout(c), (unsigned)TF_LDS_MAX);
  return VX_OK;
}

extern "C" {

const char* vx_version(void) { return "volxel_hip 0.1 (gfx950)"; }

int vx_create(int device_id, VxContext** out) {
  if (!out) return VX_ERR_INVALID;
  *out = nullptr;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0) {
    g_create_error = "vx_create: no HIP device visible (libvolxel_hip has no CPU fallback)";
    return VX_ERR_NO_DEVICE;
  }
  if (device_id < 0 || device_id >= n) {
    g_create_error = "vx_create: device ordinal out of range";
    return VX_ERR_INVALID;
  }
  VxContext* c = new VxContext();
  c->device = device_id;
  if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&c->prop, device_id) != hipSuccess ||
      hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking) != hipSuccess) {
    g_create_error = "vx_create: device initialisation failed";
    delete c;
    return VX_ERR_DEVICE;
  }
  c->stream = c->own_stream;
  {
    // lanes = pixels x frames (vx_kernels.hpp frame_group) reads per-lane frame slots from the kernel-argument segment
    // at the offsets of struct KArgs: check once per context that the compiler lays the arguments out that way
    VxParams tp{};
    DevVolume tv{};
    MultiOut tm{};
    tp.res[0] = 0x1234;
    tv.extent[0] = 0x5678u;
    for (uint32_t i = 0; i < (uint32_t)MERGE_MAX; ++i) {
      tm.out[i] = reinterpret_cast<float4*>((uintptr_t)0x100000000ull * (i + 3u) + 16u * i);
      tm.frame[i] = 0xabc00000u + 7u * i;
    }
    tm.count = MERGE_MAX;
    uint32_t* bad = nullptr;
    uint32_t hbad = 1;
    hipError_t ce = hipMalloc(&bad, 4);
    if (ce == hipSuccess) {
      hipLaunchKernelGGL(check_lane_frame_slot, dim3(1), dim3(64), 0, c->stream, tp, tv, (const float4*)nullptr, 0x9abcu, tm, bad);
      ce = hipGetLastError();
    }
    if (ce == hipSuccess) ce = hipMemcpyAsync(&hbad, bad, 4, hipMemcpyDeviceToHost, c->stream);
    if (ce == hipSuccess) ce = hipStreamSynchronize(c->stream);
    if (bad) (void)hipFree(bad);
    if (ce != hipSuccess || hbad != 0u) {
      g_create_error = ce != hipSuccess ? "vx_create: device self-check failed to run"
                                        : "vx_create: kernel-argument layout differs from struct KArgs (lane_frame_slot)";
      (void)hipStreamDestroy(c->own_stream);
      delete c;
      return VX_ERR_DEVICE;
    }
  }
  c->sw = read_switches();   // the diagnostic switches (struct Switches)
  *out = c;
  return VX_OK;
}

int vx_create_group(const int* device_ids, int n, VxContext** out) {
  if (out) *out = nullptr;
  if (!device_ids || !out || n < 1 || n > VX_GROUP_MAX) {
    g_create_error = "vx_create_group: need device_ids, 1 <= n <= 64 and out_ctx";
    return VX_ERR_INVALID;
  }
  VxContext* g = new VxContext();
  g->device = device_ids[0];
  auto drop = [g] {   // the members made so far (a group without members is not a context yet)
    for (VxContext* m : g->members) vx_destroy(m);
    delete g;
  };
  for (int i = 0; i < n; ++i) {
    VxContext* m = nullptr;
    int rc = vx_create(device_ids[i], &m);
    if (rc == VX_OK && hipEventCreateWithFlags(&m->done, hipEventDisableTiming) != hipSuccess) {
      vx_destroy(m);
      g_create_error = "event creation failed";
      rc = VX_ERR_DEVICE;
    }
    if (rc) {
      char head[80];
      snprintf(head, sizeof head, "vx_create_group: member %d (device %d): ", i, device_ids[i]);
      g_create_error = head + g_create_error;
      drop();
      return rc;
    }
    g->members.push_back(m);
  }
  // the gather runs on device_ids[0] and reads every other device's slab in place: peer access, no staging copy
  const int d0 = device_ids[0];
  for (int i = 1; i < n; ++i) {
    const int d = device_ids[i];
    if (d == d0 || std::find(device_ids + 1, device_ids + i, d) != device_ids + i) continue;
    int can = 0;
    hipError_t e = hipDeviceCanAccessPeer(&can, d0, d);
    if (e == hipSuccess && !can) {
      char buf[160];
      snprintf(buf, sizeof buf, "vx_create_group: device %d cannot access device %d as a peer", d0, d);
      g_create_error = buf;
      drop();
      return VX_ERR_NO_DEVICE;
    }
    if (e == hipSuccess) e = hipSetDevice(d0);
    if (e == hipSuccess) {
      e = hipDeviceEnablePeerAccess(d, 0);
      if (e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        e = hipSuccess;
      }
    }
    if (e != hipSuccess) {
      g_create_error = std::string("vx_create_group: peer access from device ") + std::to_string(d0) + " to " +
                       std::to_string(d) + ": " + hipGetErrorString(e);
      drop();
      return VX_ERR_DEVICE;
    }
  }
  g->prop = g->members[0]->prop;
  *out = g;
  return VX_OK;
}

void vx_destroy(VxContext* c) {
  if (!c) return;
  if (is_group(c)) {
    for (VxContext* m : c->members) vx_destroy(m);
    delete c;
    return;
  }
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  drain_events(c);
  for (auto& e : c->free_events) {
    (void)hipEventDestroy(e.a);
    (void)hipEventDestroy(e.b);
  }
  free_volume(c);
  if (c->done) (void)hipEventDestroy(c->done);
  if (c->aux_stream) (void)hipStreamDestroy(c->aux_stream);
  if (c->own_stream) (void)hipStreamDestroy(c->own_stream);
  delete c;   // every buffer and timer the context owns, on the device made current above (vx_host.hpp)
}

const char* vx_last_error(const VxContext* c) { return c ? c->err.c_str() : g_create_error.c_str(); }

int vx_set_stream(VxContext* c, void* s) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return refuse_group(c, "vx_set_stream", "each member owns its stream");
  VX_DEV(c);
  (void)hipStreamSynchronize(c->stream);
  c->stream = s ? (hipStream_t)s : c->own_stream;
  return VX_OK;
}

int vx_upload_transfer(VxContext* c, const float* rgba, uint32_t length) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_upload_transfer(m, rgba, length); });
  VX_DEV(c);
  if (!rgba || length == 0) VX_FAIL(c, VX_ERR_INVALID, "vx_upload_transfer: empty transfer function");
  // the DVR composite runs straight-line for every lane of a wave step (a lane that does not contribute adds
  // dT * rgb with dT = +0): an Inf / NaN entry would turn that 0 into NaN for lanes that never sampled it
  for (size_t i = 0; i < (size_t)length * 4; ++i)
    if (!std::isfinite(rgba[i]))
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_transfer: entry %zu component %zu is not finite", i / 4, i % 4);
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->tf.alloc(c, length)) return rc;
  VX_HIP(c, hipMemcpy(c->tf, rgba, (size_t)length * sizeof(float4), hipMemcpyHostToDevice));
  c->tf_len = length;
  c->tf_host.assign(rgba, rgba + (size_t)length * 4);
  c->vol.skip_table.stale = c->vol.lmaj_table.stale = c->vol.shadow_table.stale = true;
  c->order_builds_left = 2;
  return VX_OK;
}

int vx_upload_environment(VxContext* c, const float* rgba, uint32_t w, uint32_t h) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_upload_environment(m, rgba, w, h); });
  VX_HIP(c, hipSetDevice(c->device));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  c->env_tex.reset();
  c->env_imp.reset();
  c->env_impq.reset();
  c->env_w = c->env_h = 0;
  if (!rgba) return VX_OK;
  if (w == 0 || h == 0 || w > 16384 || h > 16384)
    VX_FAIL(c, VX_ERR_INVALID, "vx_upload_environment: bad size %ux%u", w, h);
  std::vector<float> flipped((size_t)w * h * 4);  // UNPACK_FLIP_Y_WEBGL, environment.ts:30-32
  for (uint32_t y = 0; y < h; ++y)
    memcpy(flipped.data() + (size_t)(h - 1 - y) * w * 4, rgba + (size_t)y * w * 4, (size_t)w * 16);
  if (int rc = c->env_tex.alloc(c, (size_t)w * h)) return rc;
  if (int rc = c->env_imp.alloc(c, IMP_FLOATS)) return rc;
  if (int rc = c->env_impq.alloc(c, IMPQ_QUADS)) return rc;
  VX_HIP(c, hipMemcpy(c->env_tex, flipped.data(), flipped.size() * sizeof(float), hipMemcpyHostToDevice));
  c->env_w = w;
  c->env_h = h;
  hipLaunchKernelGGL(build_importance, dim3(IMP_DIM * IMP_DIM / 256), dim3(256), 0, c->stream, c->env_tex, w, h,
                     c->env_imp);
  for (uint32_t k = 1; k < IMP_LEVELS; ++k) {
    uint32_t n = (IMP_DIM >> k) * (IMP_DIM >> k);
    hipLaunchKernelGGL(build_importance_mip, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->env_imp, k);
  }
  for (uint32_t k = 0; k + 1 < IMP_LEVELS; ++k) {
    uint32_t n = (IMP_DIM >> (k + 1)) * (IMP_DIM >> (k + 1));
    hipLaunchKernelGGL(build_importance_quads, dim3((n + 255) / 256), dim3(256), 0, c->stream, c->env_imp,
                       c->env_impq, k);
  }
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipMemcpyAsync(&c->env_avg_w, c->env_imp + (IMP_FLOATS - 1), sizeof(float),
                           hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_debug_read_importance(VxContext* c, float* out) {
  if (!c || !out) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_debug_read_importance(c->members[0], out));
  VX_DEV(c);
  if (!c->env_imp) VX_FAIL(c, VX_ERR_INVALID, "vx_debug_read_importance: no environment uploaded");
  VX_HIP(c, hipStreamSynchronize(c->stream));
  VX_HIP(c, hipMemcpy(out, c->env_imp, (size_t)IMP_FLOATS * sizeof(float), hipMemcpyDeviceToHost));
  return VX_OK;
}

int vx_set_params(VxContext* c, const VxParams* p) {
  if (!c || !p) return VX_ERR_INVALID;
  if (is_group(c)) {   // the group deals the shards: member i renders shard i of n
    if (p->shard_count != 1)
      VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: a device group shards itself; pass shard_count 1, not %d", p->shard_count);
    return fan_out(c, [&](VxContext* m, size_t i) {
      VxParams q = *p;
      q.shard_rank = (int32_t)i;
      q.shard_count = (int32_t)c->members.size();
      return vx_set_params(m, &q);
    });
  }
  VX_DEV(c);
  if (p->render_mode < VX_MODE_DEFAULT || p->render_mode > VX_MODE_MINIP)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: unknown render mode %d", p->render_mode);
  if (p->shard_count < 1 || p->shard_rank < 0 || p->shard_rank >= p->shard_count)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: bad shard %d/%d", p->shard_rank, p->shard_count);
  if (p->use_env != 0 && p->use_env != 1) VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: use_env must be 0 or 1");
  if (c->W && ((uint32_t)p->res[0] != c->W || (uint32_t)p->res[1] != c->H))
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: res %dx%d differs from vx_resize %ux%u", p->res[0],
            p->res[1], c->W, c->H);
  // the projections sample as DVR does: the same checks
  const bool marches = p->render_mode == VX_MODE_DVR || p->render_mode == VX_MODE_DVR_PHONG || proj_mode(p->render_mode);
  if (marches && !(p->dvr_step_voxels > 0.0f))
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_step_voxels must be > 0");
  // the kernels count steps in fp32 (t_k = fma(k, dt, t0)): beyond 2^24 the count stops advancing
  if (marches && (p->dvr_max_steps < 0 || p->dvr_max_steps > (1 << 24)))
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_max_steps %d outside [0, 2^24]", p->dvr_max_steps);
  if (p->dvr_shadow_stride != 0 && p->dvr_shadow_stride != 1 && p->dvr_shadow_stride != 2 && p->dvr_shadow_stride != 4)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_shadow_stride must be 0, 1, 2 or 4, not %d", p->dvr_shadow_stride);
  if (p->dvr_shadow_stride != 0 && p->render_mode == VX_MODE_DVR_PHONG)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_shadow_stride %d with VX_MODE_DVR_PHONG (shadows serve plain DVR)",
            p->dvr_shadow_stride);
  if (p->dvr_shadow_stride != 0 && proj_mode(p->render_mode))
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_shadow_stride %d with an intensity projection (shadows serve plain DVR)",
            p->dvr_shadow_stride);
  if (p->dvr_shadow_stride != 0 && p->render_mode == VX_MODE_DVR && p->use_env != 0)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_params: dvr_shadow_stride %d with use_env = 1 (an environment map has no single light "
            "direction)", p->dvr_shadow_stride);
  bool reshard = !c->has_params || p->shard_count != c->params.shard_count ||
                 p->shard_rank != c->params.shard_rank;
  if (!c->has_params || memcmp(&c->params, p, sizeof(VxParams)) != 0) c->order_builds_left = 2;
  c->params = *p;
  c->has_params = true;
  if (reshard && c->W) {
    VX_HIP(c, hipStreamSynchronize(c->stream));
    return alloc_framebuffers(c);
  }
  return VX_OK;
}

int vx_resize(VxContext* c, uint32_t w, uint32_t h) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_resize(m, w, h); });
  if (w == 0 || h == 0 || w > 16384 || h > 16384) VX_FAIL(c, VX_ERR_INVALID, "vx_resize: bad size %ux%u", w, h);
  VX_HIP(c, hipSetDevice(c->device));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if ((w != c->W || h != c->H) && c->tile_perm) {  // a dealing order belongs to one image size
    c->tile_perm.reset();
    c->tile_perm_n = 0;
  }
  c->W = w;
  c->H = h;
  return alloc_framebuffers(c);
}

int vx_render_frame(VxContext* c, uint32_t frame_index, float sample_weight) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_render_frame(m, frame_index, sample_weight); });
  VX_DEV(c);
  int rc = prepare_render(c);
  if (rc) return rc;
  MultiOut mo{};
  mo.count = 1;
  mo.out[0] = c->slab;
  mo.dc[0] = c->dc;
  mo.frame[0] = frame_index;
  const LaunchPlan lp = plan_launch(c, mo);
  EventPair ev;
  if ((rc = take_events(c, ev))) return rc;
  VX_HIP(c, hipEventRecord(ev.a, c->stream));
  rc = launch_planned(c, lp, mo, sample_weight);
  VX_HIP(c, hipEventRecord(ev.b, c->stream));
  c->pending_events.push_back(ev);
  if (rc) return rc;
  if (lp.kernel == Kernel::GENERIC) c->order_builds_left = 0;   // render_generic runs its blocks in launch order
  else if (c->order_builds_left > 0) {
    c->order_builds_left--;
    hipLaunchKernelGGL(build_order, dim3(1), dim3(1024), 0, c->stream, c->dc, c->order, frame_blocks(c));
    VX_HIP(c, hipGetLastError());
    c->miss.split_stale = true;
  }
  c->note_launch(1);
  return VX_OK;
}

// `count` accumulation frames first_frame.. with their sample weights, up to `in_flight` of them in one launch (frames
// are independent given their index; only the running mean is ordered).  A launch either folds the running mean of its
// frames itself (plan_launch's fuse rule) or writes per-frame result slabs that merge_results then blends in frame
// order -- bit-identical to count vx_render_frame calls either way.  Hides the latency-bound tail of one frame behind
// the bulk of the next ones.
int vx_render_frames(VxContext* c, uint32_t first_frame, uint32_t count, const float* weights, int in_flight) {
  if (!c || (!weights && count)) return VX_ERR_INVALID;
  if (is_group(c))   // enqueued on every member's stream, no wait: distinct devices render concurrently
    return fan_out(c, [&](VxContext* m, size_t) { return vx_render_frames(m, first_frame, count, weights, in_flight); });
  VX_DEV(c);
  if (in_flight > MERGE_MAX) in_flight = MERGE_MAX;
  uint32_t done = 0;
  // frames that still refresh the launch order, and the degenerate cases, go one by one
  while (done < count && (in_flight <= 1 || c->order_builds_left > 0 || !c->has_params || c->dc_waves == 0)) {
    int rc = vx_render_frame(c, first_frame + done, weights[done]);
    if (rc) return rc;
    ++done;
  }
  if (done == count) return VX_OK;
  int rc = prepare_render(c, true);
  if (rc) return rc;
  if ((rc = ensure_pipes(c, (uint32_t)in_flight))) return rc;
  const uint32_t nq = (uint32_t)c->slab_quads;
  while (done < count) {
    const uint32_t n = std::min(count - done, (uint32_t)in_flight);
    MultiOut mo{};
    MergeArgs ma{};
    mo.count = n;
    ma.count = n;
    for (uint32_t i = 0; i < n; ++i) {
      mo.out[i] = c->pipe_result_pool + i * c->pipe_quads;
      mo.dc[i] = c->pipe_dc_pool + i * c->pipe_waves;
      mo.frame[i] = first_frame + done + i;
      ma.result[i] = mo.out[i];
      ma.weight[i] = weights[done + i];
    }
    const LaunchPlan lp = plan_launch(c, mo);
    if (lp.fuse) {
      bool zero = false;
      for (uint32_t i = 0; i < n; ++i) {
        mo.weight[i] = ma.weight[i];
        zero = zero || ma.weight[i] == 0.0f;
      }
      mo.fuse = zero ? 2u : 1u;
      mo.accum = c->slab;
    }
    EventPair ev;
    if ((rc = take_events(c, ev))) return rc;
    VX_HIP(c, hipEventRecord(ev.a, c->stream));
    rc = launch_planned(c, lp, mo, 0.0f);
    VX_HIP(c, hipEventRecord(ev.b, c->stream));   // the render kernel alone; the blend is timed apart
    c->pending_events.push_back(ev);
    if (rc) return rc;
    if (!lp.fuse) {
      EventPair em;
      if ((rc = take_events(c, em))) return rc;
      em.merge = true;
      VX_HIP(c, hipEventRecord(em.a, c->stream));
      hipLaunchKernelGGL(merge_results, dim3((nq + 255) / 256), dim3(256), 0, c->stream, c->slab, ma, nq);
      VX_HIP(c, hipGetLastError());
      VX_HIP(c, hipEventRecord(em.b, c->stream));
      c->pending_events.push_back(em);
      c->merge_launches += 1;
    }
    done += n;
    c->note_launch(n);
  }
  return VX_OK;
}

int vx_finish(VxContext* c) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_finish(m); });
  VX_DEV(c);
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_detile(VxContext* c, const void* gathered, void* image_out) {
  if (!c || !gathered || !image_out) return VX_ERR_INVALID;
  if (is_group(c)) return refuse_group(c, "vx_detile", "it has no single slab; vx_read_* gather the members");
  VX_DEV(c);
  std::vector<const float4*> t(c->tm.shard_count);
  for (size_t s = 0; s < t.size(); ++s) t[s] = (const float4*)gathered + s * c->slab_quads;
  int rc = set_slab_table(c, t);
  return rc ? rc : launch_detile(c, (float4*)image_out);
}

int vx_read_accum(VxContext* c, float* out) {
  if (!c || !out) return VX_ERR_INVALID;
  VX_DEV(c);
  VxContext* d = nullptr;
  int rc = compose_image(c, d);
  if (rc) return rc;
  VX_HIP(c, hipMemcpyAsync(out, d->image, (size_t)d->W * d->H * sizeof(float4), hipMemcpyDeviceToHost, d->stream));
  VX_HIP(c, hipStreamSynchronize(d->stream));
  return VX_OK;
}

int vx_read_display_scaled(VxContext* c, uint8_t* out, uint32_t ow, uint32_t oh, float exposure, float gamma) {
  if (!c || !out) return VX_ERR_INVALID;
  VX_DEV(c);
  if (ow == 0 || oh == 0 || (uint64_t)ow * oh > (1ull << 28)) {
    c->err = "vx_read_display_scaled: bad canvas size";
    return VX_ERR_INVALID;
  }
  VxContext* d = nullptr;
  int rc = compose_image(c, d);
  if (rc) return rc;
  uint32_t n = ow * oh;
  if ((rc = d->display.ensure(c, n))) return rc;
  hipLaunchKernelGGL(blit_rgba8, dim3((n + 255) / 256), dim3(256), 0, d->stream, d->image, d->display, d->W, d->H,
                     ow, oh, exposure, gamma);
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipMemcpyAsync(out, d->display, (size_t)n * 4, hipMemcpyDeviceToHost, d->stream));
  VX_HIP(c, hipStreamSynchronize(d->stream));
  return VX_OK;
}

int vx_read_display(VxContext* c, uint8_t* out, float exposure, float gamma) {
  if (!c) return VX_ERR_INVALID;
  const VxContext* d = is_group(c) ? c->members[0] : c;
  return vx_read_display_scaled(c, out, d->W, d->H, exposure, gamma);
}

int vx_probe_tile_costs(VxContext* c, uint32_t* costs, uint32_t n) {
  if (!c || !costs) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_probe_tile_costs(c->members[0], costs, n));   // every member derives the same costs
  VX_DEV(c);
  if (!c->vol.has_volume) VX_FAIL(c, VX_ERR_NO_VOLUME, "vx_probe_tile_costs: no volume uploaded");
  if (!c->has_params || !c->tf || !c->W) VX_FAIL(c, VX_ERR_INVALID, "vx_probe_tile_costs: params, transfer function and size first");
  if (n != c->tm.n_tiles) VX_FAIL(c, VX_ERR_INVALID, "vx_probe_tile_costs: the image has %u tiles, not %u", c->tm.n_tiles, n);
  int rc = prepare_render(c);   // skip mask, environment pointers
  if (rc) return rc;
  uint32_t* d = nullptr;
  VX_HIP(c, hipMalloc(&d, (size_t)n * 4));
  with_layout(eff_layout(c), [&](auto tag) {
    hipLaunchKernelGGL((probe_tile_costs<decltype(tag)::value>), dim3(n), dim3(64), 0, c->stream, c->params, c->vol.dv, c->tf, c->tf_len,
                       c->tm, d);
  });
  hipError_t le = hipGetLastError();
  if (le == hipSuccess) le = hipMemcpyAsync(costs, d, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (le == hipSuccess) le = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (le != hipSuccess) VX_FAIL(c, VX_ERR_DEVICE, "vx_probe_tile_costs: %s", hipGetErrorString(le));
  return VX_OK;
}

int vx_set_tile_order(VxContext* c, const uint32_t* perm, uint32_t n) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_set_tile_order(m, perm, n); });
  VX_DEV(c);
  if (!c->W) VX_FAIL(c, VX_ERR_INVALID, "vx_set_tile_order: vx_resize first");
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (perm) {
    if (n != c->tm.n_tiles) VX_FAIL(c, VX_ERR_INVALID, "vx_set_tile_order: the image has %u tiles, not %u", c->tm.n_tiles, n);
    std::vector<uint32_t> both(2 * (size_t)n, 0xffffffffu);
    for (uint32_t pos = 0; pos < n; ++pos) {
      uint32_t t = perm[pos];
      if (t >= n || both[n + t] != 0xffffffffu) VX_FAIL(c, VX_ERR_INVALID, "vx_set_tile_order: not a permutation of the tiles");
      both[pos] = t;
      both[n + t] = pos;
    }
    c->tile_perm_n = 0;
    if (int rc = c->tile_perm.alloc(c, both.size())) return rc;
    VX_HIP(c, hipMemcpy(c->tile_perm, both.data(), both.size() * 4, hipMemcpyHostToDevice));
    c->tile_perm_n = n;
    c->tile_perm_host.assign(both.begin(), both.begin() + n);
  } else {
    c->tile_perm.reset();
    c->tile_perm_n = 0;
  }
  update_tilemap(c);
  if (c->slab) VX_HIP(c, hipMemsetAsync(c->slab, 0, c->slab_quads * sizeof(float4), c->stream));  // other tiles now
  c->order_builds_left = 2;
  return VX_OK;
}

int vx_render_size(VxContext* c, uint32_t* w, uint32_t* h) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) c = c->members[0];
  if (w) *w = c->W;
  if (h) *h = c->H;
  return VX_OK;
}

int vx_slab_info(VxContext* c, uint64_t* slab_floats, uint32_t* tiles_per_shard) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return refuse_group(c, "vx_slab_info", "it has no single slab");
  if (slab_floats) *slab_floats = (uint64_t)c->slab_quads * 4u;
  if (tiles_per_shard) *tiles_per_shard = c->tm.tiles_per_shard;
  return VX_OK;
}

int vx_slab_device_ptr(VxContext* c, void** p) {
  if (!c || !p) return VX_ERR_INVALID;
  if (is_group(c)) return refuse_group(c, "vx_slab_device_ptr", "it has no single slab");
  *p = c->slab;
  return VX_OK;
}

int vx_get_counters(VxContext* c, VxCounters* out) {
  if (!c || !out) return VX_ERR_INVALID;
  if (is_group(c)) {   // work summed; frames from member 0 (all render the same frames); times: the slowest member
    VxCounters t{};
    return fan_out(c, [&](VxContext* m, size_t i) {
      VxCounters k{};
      if (int rc = vx_get_counters(m, &k)) return rc;
      if (i == 0) {
        t = k;
      } else {
        t.samples += k.samples;
        t.rays += k.rays;
        t.pixels += k.pixels;
        t.skip_steps += k.skip_steps;
        t.grad_samples += k.grad_samples;
        t.tf_samples += k.tf_samples;
        t.lane_slots += k.lane_slots;
        t.active_lane_slots += k.active_lane_slots;
        t.gathers += k.gathers;
        t.lds_reads += k.lds_reads;
        t.launches += k.launches;
        t.merge_launches += k.merge_launches;
        t.kernel_ms = std::max(t.kernel_ms, k.kernel_ms);
        t.last_kernel_ms = std::max(t.last_kernel_ms, k.last_kernel_ms);
        t.merge_ms = std::max(t.merge_ms, k.merge_ms);
      }
      if (i + 1 == c->members.size()) *out = t;
      return VX_OK;
    });
  }
  VX_DEV(c);
  VX_HIP(c, hipStreamSynchronize(c->stream));
  drain_events(c);
  int rc = fold_counters(c);
  if (rc) return rc;
  out->samples = c->base.samples;
  out->rays = c->base.rays;
  out->pixels = c->base.pixels;
  out->skip_steps = c->base.skip_steps;
  out->grad_samples = c->base.grad_samples;
  out->lane_slots = c->base.lane_slots;
  out->launches = c->launches;
  out->frames = c->frames;
  out->kernel_ms = c->kernel_ms;
  out->last_kernel_ms = c->last_kernel_ms;
  out->gathers = c->base.gathers;
  out->lds_reads = c->base.lds_reads;
  out->merge_ms = c->merge_ms;
  out->min_launch_frames = c->min_launch_frames;
  out->max_launch_frames = c->max_launch_frames;
  out->tf_samples = c->base.tf_samples;
  out->active_lane_slots = c->base.active_lane_slots;
  out->merge_launches = c->merge_launches;
  return VX_OK;
}

int vx_reset_counters(VxContext* c) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_reset_counters(m); });
  VX_DEV(c);
  VX_HIP(c, hipStreamSynchronize(c->stream));
  drain_events(c);
  {
    int rc = fold_counters(c);   // zeroes every record array (accumulator and multi-frame slots)
    if (rc) return rc;
  }
  c->base = VxCounters{};
  c->kernel_ms = c->last_kernel_ms = c->merge_ms = 0.0;
  c->launches = 0;
  c->frames = 0;
  c->merge_launches = 0;
  c->min_launch_frames = c->max_launch_frames = 0;
  return VX_OK;
}

int vx_device_info(VxContext* c, char* name, uint32_t cap, uint32_t* cus, uint64_t* hbm) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) c = c->members[0];
  if (name && cap) {
    snprintf(name, cap, "%s (%s)", c->prop.name, c->prop.gcnArchName);
  }
  if (cus) *cus = (uint32_t)c->prop.multiProcessorCount;
  if (hbm) *hbm = (uint64_t)c->prop.totalGlobalMem;
  return VX_OK;
}

// test hook: the host-side skip mask for a brick grid / TF / uniforms (pure CPU, no context).
// bits_out must hold ((prod(dims)+31)/32) words; call with bits_out == NULL to get level / dims.
int vx_debug_build_skip_mask(const uint32_t* range_packed, const uint32_t brick_count[3], const float* tf_rgba,
                             uint32_t tf_len, const VxParams* p, uint32_t* bits_out, uint32_t* level_out,
                             uint32_t dims_out[3]) {
  if (!range_packed || !brick_count || !tf_rgba || !tf_len || !p) return VX_ERR_INVALID;
  uint32_t extent[3] = {brick_count[0] * 8u, brick_count[1] * 8u, brick_count[2] * 8u};
  std::vector<uint32_t> bits;
  int level = 1;
  uint32_t md[3];
  compute_skip_mask(*p, range_packed, brick_count, extent, tf_rgba, tf_len, bits, level, md);
  if (level_out) *level_out = (uint32_t)level;
  if (dims_out) { dims_out[0] = md[0]; dims_out[1] = md[1]; dims_out[2] = md[2]; }
  if (bits_out) memcpy(bits_out, bits.data(), bits.size() * 4);
  return VX_OK;
}

// test hook: the host-built density bounds of range skipping (pure CPU, no context), {lo, hi} per macro cell
int vx_debug_build_projection_bounds(const uint32_t* range_packed, const uint32_t brick_count[3], const VxParams* p,
                                     float* bounds_out, uint32_t* level_out, uint32_t dims_out[3]) {
  if (!range_packed || !brick_count || !p) return VX_ERR_INVALID;
  uint32_t extent[3] = {brick_count[0] * 8u, brick_count[1] * 8u, brick_count[2] * 8u};
  std::vector<float> lohi;
  int level = 1;
  uint32_t md[3];
  compute_projection_bounds(*p, range_packed, brick_count, extent, lohi, level, md);
  if (level_out) *level_out = (uint32_t)level;
  if (dims_out) { dims_out[0] = md[0]; dims_out[1] = md[1]; dims_out[2] = md[2]; }
  if (bounds_out) memcpy(bounds_out, lohi.data(), lohi.size() * sizeof(float));
  return VX_OK;
}

// test hook: the host's classification of the image's 16x16-pixel blocks (pure CPU, no context), under the VX_DVR_MISS switch
int vx_debug_classify_miss_blocks(const VxParams* p, uint32_t width, uint32_t height, uint8_t* flags_out, uint32_t* n_out) {
  if (!p || width == 0 || height == 0 || width > 16384 || height > 16384) return VX_ERR_INVALID;
  std::vector<uint8_t> flags;
  uint32_t n = 0;
  if (dvr_miss_switch()) n = classify_miss_blocks(*p, width, height, flags);
  else flags.assign((size_t)((width + 15u) / 16u) * ((height + 15u) / 16u), 0);
  if (flags_out) memcpy(flags_out, flags.data(), flags.size());
  if (n_out) *n_out = n;
  return VX_OK;
}

// test hook: the blocks per frame slot the last render launch gave the LDS-window kernel (or whichever single kernel ran) and
// render_dvr_miss
int vx_debug_last_launch_blocks(VxContext* c, uint32_t* heavy, uint32_t* miss) {
  if (!c) return VX_ERR_INVALID;
  uint32_t h = 0, m = 0;
  for (const VxContext* k : is_group(c) ? c->members : std::vector<VxContext*>{c}) {
    h += k->miss.last_heavy;
    m += k->miss.last_miss;
  }
  if (heavy) *heavy = h;
  if (miss) *miss = m;
  return VX_OK;
}

// test hook: random.glsl on the device
int vx_debug_rng(VxContext* c, int op, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out) {
  if (!c || !a || !out || n == 0 || n > 65536u || op < 0 || op > 4 || (op == 0 && !b)) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_debug_rng(c->members[0], op, a, b, n, out));
  VX_DEV(c);
  const uint32_t n_in = op < 2 ? n : 1u;
  uint32_t *da = nullptr, *db = nullptr, *dout = nullptr;
  hipError_t e = hipMalloc(&da, (size_t)n_in * 4);
  if (e == hipSuccess) e = hipMalloc(&db, (size_t)n_in * 4);
  if (e == hipSuccess) e = hipMalloc(&dout, (size_t)n * 4);
  if (e == hipSuccess) e = hipMemcpyAsync(da, a, (size_t)n_in * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess && op == 0) e = hipMemcpyAsync(db, b, (size_t)n_in * 4, hipMemcpyHostToDevice, c->stream);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(debug_rng, dim3((n + 255) / 256), dim3(256), 0, c->stream, op, da, db, n, dout);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipMemcpyAsync(out, dout, (size_t)n * 4, hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(da);
  (void)hipFree(db);
  (void)hipFree(dout);
  if (e != hipSuccess) VX_FAIL(c, VX_ERR_DEVICE, "vx_debug_rng: %s", hipGetErrorString(e));
  return VX_OK;
}

// measurement hook: what the vector ALUs of this device sustain -- clocks (nominal) per wave64 VALU instruction per SIMD
int vx_probe_valu_rate(VxContext* c, double* clk_out, uint32_t* clock_khz_out) {
  if (!c || !clk_out) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_probe_valu_rate(c->members[0], clk_out, clock_khz_out));
  VX_DEV(c);
  float* sink = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipMalloc(&sink, 4);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  const int cus = c->prop.multiProcessorCount, iters = 4096, blocks = cus * 8;   // 32 waves per CU = 8 per SIMD
  float ms = 0.f;
  for (int rep = 0; rep < 3 && e == hipSuccess; ++rep) {
    e = hipEventRecord(e0, c->stream);
    hipLaunchKernelGGL(probe_valu_rate, dim3(blocks), dim3(256), 0, c->stream, sink, iters, 1.0001f, 0.5f);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(sink);
  if (e != hipSuccess) VX_FAIL(c, VX_ERR_DEVICE, "vx_probe_valu_rate: %s", hipGetErrorString(e));
  const double khz = (double)c->prop.clockRate;
  const double inst_per_simd = (double)iters * 16.0 * 8.0;   // 8 waves per SIMD, 16 FMAs per iteration each
  *clk_out = (ms * 1e-3 * khz * 1e3) / inst_per_simd;
  if (clock_khz_out) *clock_khz_out = (uint32_t)c->prop.clockRate;
  return VX_OK;
}

// measurement hook: L1 gather rate for a given number of distinct lines per gather instruction
int vx_probe_gather_rate(VxContext* c, uint32_t lines, uint32_t distinct, double* clk_out, uint32_t* clock_khz_out) {
  if (!c || !clk_out || lines < 1u || lines > 64u || distinct < 1u || distinct > lines) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_probe_gather_rate(c->members[0], lines, distinct, clk_out, clock_khz_out));
  VX_DEV(c);
  float4* table = nullptr;
  float* sink = nullptr;
  hipEvent_t e0 = nullptr, e1 = nullptr;
  hipError_t e = hipMalloc(&table, 128u * 128u);   // 128 lines = 16 KiB: L1 resident
  if (e == hipSuccess) e = hipMalloc(&sink, 4);
  if (e == hipSuccess) e = hipMemsetAsync(table, 0, 128u * 128u, c->stream);
  if (e == hipSuccess) e = hipEventCreate(&e0);
  if (e == hipSuccess) e = hipEventCreate(&e1);
  const int cus = c->prop.multiProcessorCount, iters = 512, blocks = cus * 5;   // 20 waves per CU
  float ms = 0.f;
  for (int rep = 0; rep < 3 && e == hipSuccess; ++rep) {   // the last repetition is the one reported
    e = hipEventRecord(e0, c->stream);
    hipLaunchKernelGGL(probe_gather_rate, dim3(blocks), dim3(256), 0, c->stream, table, lines, distinct, iters, sink);
    if (e == hipSuccess) e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(e1, c->stream);
    if (e == hipSuccess) e = hipEventSynchronize(e1);
    if (e == hipSuccess) e = hipEventElapsedTime(&ms, e0, e1);
  }
  if (e0) (void)hipEventDestroy(e0);
  if (e1) (void)hipEventDestroy(e1);
  (void)hipFree(table);
  (void)hipFree(sink);
  if (e != hipSuccess) VX_FAIL(c, VX_ERR_DEVICE, "vx_probe_gather_rate: %s", hipGetErrorString(e));
  const double khz = (double)c->prop.clockRate;
  const double gathers_per_cu = (double)blocks * 4.0 * iters * 8.0 / cus;
  *clk_out = (ms * 1e-3 * khz * 1e3) / gathers_per_cu;
  if (clock_khz_out) *clock_khz_out = (uint32_t)c->prop.clockRate;
  return VX_OK;
}

// measurement hook: distinct lines per gather of the tuned cellquad DVR march (one frame, nothing is stored)
int vx_probe_gather_spread(VxContext* c, uint32_t frame_index, uint64_t out3[3]) {
  if (!c || !out3) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_probe_gather_spread(c->members[0], frame_index, out3));
  VX_DEV(c);
  int rc = prepare_render(c);
  if (rc) return rc;
  MultiOut mo{};
  mo.count = 1;
  mo.out[0] = c->slab;   // never written by the probe build
  mo.frame[0] = frame_index;
  const LaunchPlan lp = plan_launch(c, mo, true);
  if (lp.kernel != Kernel::DVR_CQ)
    VX_FAIL(c, VX_ERR_INVALID, "vx_probe_gather_spread: needs render_mode dvr on the cellquad layout");
  const size_t waves = (size_t)frame_blocks(c) * 4u;
  DevCounters* d = nullptr;
  VX_HIP(c, hipMalloc(&d, waves * sizeof(DevCounters)));
  hipError_t e = hipMemsetAsync(d, 0, waves * sizeof(DevCounters), c->stream);
  mo.dc[0] = d;
  if (e == hipSuccess && (rc = launch_planned(c, lp, mo, 0.0f))) {
    (void)hipFree(d);
    return rc;
  }
  std::vector<DevCounters> h(waves);
  if (e == hipSuccess) e = hipMemcpyAsync(h.data(), d, waves * sizeof(DevCounters), hipMemcpyDeviceToHost, c->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
  (void)hipFree(d);
  if (e != hipSuccess) VX_FAIL(c, VX_ERR_DEVICE, "vx_probe_gather_spread: %s", hipGetErrorString(e));
  out3[0] = out3[1] = out3[2] = 0;
  for (const auto& w : h) {
    out3[0] += w.gathers / 2u;   // q0 gathers (q1 repeats the pattern one slice further)
    out3[1] += w.rays;           // wave-wide distinct lines, summed over the q0 gathers
    out3[2] += w.pixels;         // look-ups of the 16 lane quads, summed over the q0 gathers
  }
  return VX_OK;
}

int vx_shadow_stats(VxContext* c, uint64_t* builds, uint64_t* light_samples, double* last_build_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_shadow_stats(c->members[0], builds, light_samples, last_build_ms));
  VX_DEV(c);
  unsigned long long n = 0;
  double ms = 0.0;
  if (c->shadow_builds) {
    VX_HIP(c, hipStreamSynchronize(c->stream));
    VX_HIP(c, hipMemcpy(&n, c->shadow_count_dev, sizeof n, hipMemcpyDeviceToHost));
    if (int rc = c->shadow_timer.read(c)) return rc;
    ms = c->shadow_timer.ms[0];
  }
  if (builds) *builds = c->shadow_builds;
  if (light_samples) *light_samples = n;
  if (last_build_ms) *last_build_ms = ms;
  return VX_OK;
}

int vx_debug_read_shadow_grid(VxContext* c, float* out, uint32_t dims_out[3]) {
  if (!c || !dims_out) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_debug_read_shadow_grid(c->members[0], out, dims_out));
  VX_DEV(c);
  if (!c->vol.shadow.t) VX_FAIL(c, VX_ERR_INVALID, "vx_debug_read_shadow_grid: no light grid built since the last upload");
  for (int i = 0; i < 3; ++i) dims_out[i] = c->vol.shadow.n[i];
  if (out) {
    VX_HIP(c, hipStreamSynchronize(c->stream));
    VX_HIP(c, hipMemcpy(out, c->vol.shadow.t, (size_t)c->vol.shadow.n[0] * c->vol.shadow.n[1] * c->vol.shadow.n[2] * sizeof(float),
                        hipMemcpyDeviceToHost));
  }
  return VX_OK;
}

// test hook (not part of the reference boundary): the device's unorm8 decode table
int vx_debug_unorm_table(VxContext* c, float* out256) {
  if (!c || !out256) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_debug_unorm_table(c->members[0], out256));
  VX_DEV(c);
  float* d = nullptr;
  VX_HIP(c, hipMalloc(&d, 256 * sizeof(float)));
  hipLaunchKernelGGL(unorm_table, dim3(1), dim3(256), 0, c->stream, d);
  VX_HIP(c, hipMemcpyAsync(out256, d, 256 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  (void)hipFree(d);
  return VX_OK;
}

}  // extern "C"
