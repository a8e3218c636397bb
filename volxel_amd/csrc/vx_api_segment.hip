// vx_api_segment.hip -- the segment unit of the host layer (units: DESIGN.md section 4.1): the segment chain -- seeded region
// growing, the mask's read-back, slice overlay and view, the edits, the threshold, the islands, the distance field with the
// millimetre margins, the segment store with its set operations, comparison and label map, and the histograms.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "vx_segment.hpp"
#include "vx_segedit.hpp"
#include "vx_islands.hpp"
#include "vx_distance.hpp"
#include "vx_segstore.hpp"
#include "vx_histogram.hpp"
#include "vx_context.hpp"

using namespace vx;

namespace {

// ---- segmentation (vx_segment): seg_predicate, the flood rounds, seg_stats / seg_sum (vx_segment.hpp) ----------------------
// rounds between host read-backs of the next worklist's length: 1, 2, 4, ... up to Switches::seg_check_max (64; NOTEBOOK
// "Segmentation" compares caps).  A queued round that finds its worklist empty exits at once (one launch boundary, a few
// microseconds); a read-back is a host round trip.

// the device buffers of the brick grid, carved from one allocation (sizes in DESIGN.md / INTEGRATION.md's memory bill)
static int ensure_segment(VxContext* c) {
  if (c->vol.seg_alloc) return VX_OK;
  const uint32_t nb = c->vol.dv.bc[0] * c->vol.dv.bc[1] * c->vol.dv.bc[2];
  SegDev& s = c->vol.seg;
  const int rc = carve(c, c->vol.seg_alloc, [&](Carve& k) {
    s.pred = k.take<uint64_t>((size_t)nb * 8u);
    s.seg = k.take<uint64_t>((size_t)nb * 8u);
    // `partial` stays immediately behind `seg`: the masked LDS-window staging reads the dword right behind the mask for the
    // zero chunk behind the last brick -- the first of `partial`, inside this allocation -- and drops its bits
    // (vx_dvr_lds_march.inc)
    s.partial = k.take<double>(nb);
    s.st = k.take<SegStats>();
    s.any = k.take<uint32_t>(nb);
    s.stamp = k.take<uint32_t>(nb);
    s.list[0] = k.take<uint32_t>(nb);
    s.list[1] = k.take<uint32_t>(nb);
    s.cnt = k.take<uint32_t>(4);
  });
  if (rc) return rc;
  for (int a = 0; a < 3; ++a) s.bc[a] = c->vol.dv.bc[a];
  s.nb = nb;
  return VX_OK;
}

static void launch_seg_predicate(VxContext* c, const SegPredParams& pp) {
  const VxParams& p = c->params;
  const uint32_t blocks = std::min<uint32_t>((c->vol.seg.nb + 3u) / 4u, 4096u);
  with_layout(slice_layout(c), [&](auto lay) {
    constexpr int LAY = decltype(lay)::value;
    hipLaunchKernelGGL((seg_predicate<LAY>), dim3(blocks), dim3(256), 0, c->stream, c->vol.dv, p.volume_density_scale, p.volume_inv_maj,
                       pp, c->vol.seg);
  });
}

static SegPredParams seg_pred_params(float lo, float hi, const VoxelBox& b) {
  return SegPredParams{lo, hi, {b.lo[0], b.lo[1], b.lo[2]}, {b.hi[0], b.hi[1], b.hi[2]}};
}

// the brick, the z slice and the bit of a voxel
static SegSeed seg_seed_of(const SegDev& s, const uint32_t v[3]) {
  return SegSeed{((v[2] >> 3) * s.bc[1] + (v[1] >> 3)) * s.bc[0] + (v[0] >> 3), v[2] & 7u, 1ull << (((v[1] & 7u) << 3) | (v[0] & 7u))};
}

static void launch_seg_flood(VxContext* c, const SegDev& s, int conn, const SegSeed& seed, uint32_t round) {
  const uint32_t blocks = std::min<uint32_t>((s.nb + 255u) / 256u, 1024u);
  with_conn(conn, [&](auto k) {
    hipLaunchKernelGGL((seg_flood<decltype(k)::value>), dim3(blocks), dim3(256), 0, c->stream, s, seed, round);
  });
}

// the rounds of a flood on the view s (vx_segment: the segment; vx_segment_edit: the background of fill holes), from a round-0
// worklist that is already on the device: queued in batches of 1, 2, 4, ... SEG_CHECK_MAX, the next worklist's length read back
// after each batch.  Ends synchronised; *launched counts the flood launches.
static int run_seg_flood(VxContext* c, const SegDev& s, int conn, const SegSeed& seed, uint64_t cap, bool* converged,
                         uint64_t* launched_out) {
  uint64_t launched = 0;
  uint32_t batch = 1, next = 1;
  *converged = false;
  while (true) {
    const uint64_t k = std::min<uint64_t>(batch, cap - launched);
    for (uint64_t i = 0; i < k; ++i) launch_seg_flood(c, s, conn, seed, (uint32_t)(launched + i));
    VX_HIP(c, hipGetLastError());
    launched += k;
    VX_HIP(c, hipMemcpyAsync(&next, s.cnt + launched % 3u, sizeof next, hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipStreamSynchronize(c->stream));
    if (next == 0u) {
      *converged = true;
      break;
    }
    if (launched >= cap) break;
    batch = std::min(batch * 2u, c->sw.seg_check_max);
  }
  if (launched_out) *launched_out = launched;
  return VX_OK;
}

static void launch_seg_stats(VxContext* c) {
  const VxParams& p = c->params;
  const uint32_t blocks = std::min<uint32_t>((c->vol.seg.nb + 3u) / 4u, 4096u);
  with_layout(slice_layout(c), [&](auto lay) {
    constexpr int LAY = decltype(lay)::value;
    hipLaunchKernelGGL((seg_stats<LAY>), dim3(blocks), dim3(256), 0, c->stream, c->vol.dv, p.volume_density_scale, p.volume_inv_maj,
                       c->vol.seg);
  });
  hipLaunchKernelGGL(seg_sum, dim3(1), dim3(1024), 0, c->stream, c->vol.seg);
}

static float seg_key_float(uint32_t k) {
  const uint32_t u = (k & 0x80000000u) ? (k & 0x7fffffffu) : ~k;
  float f;
  memcpy(&f, &u, sizeof f);
  return f;
}

// the count, bounding box and density statistics of a result; rounds, brick_visits and converged are the caller's
static VxSegmentResult seg_result(const SegStats& st) {
  VxSegmentResult r{};
  r.count = st.count;
  if (st.count) {
    for (int a = 0; a < 3; ++a) {
      r.bbox_lo[a] = st.lo[a];
      r.bbox_hi[a] = st.hi[a];
    }
    r.d_min = seg_key_float(st.dmin);
    r.d_max = seg_key_float(st.dmax);
    r.d_sum = st.sum;
  }
  return r;
}

// The statistics of the mask in SegDev::seg, behind whatever wrote it on the stream: sed_reset, seg_stats / seg_sum (three
// launches), event `done` of the caller's timer behind them, the read-back.  Ends synchronised.
template <int N>
static int seg_mask_stats(VxContext* c, StageTimer<N>& timer, int done, SegStats* st) {
  hipLaunchKernelGGL(sed_reset, dim3(1), dim3(64), 0, c->stream, c->vol.seg, 0u);
  launch_seg_stats(c);
  VX_HIP(c, hipGetLastError());
  if (int rc = timer.mark(c, done)) return rc;
  VX_HIP(c, hipMemcpyAsync(st, c->vol.seg.st, sizeof *st, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

// ---- segment edits (vx_segment_edit, vx_segment_write_mask; kernels in vx_segedit.hpp) ---------------------------------------
// the scratch of the edits: two masks of nb * 8 words (1 bit per voxel each) and the fill's nb "any background" flags
static int ensure_segedit(VxContext* c) {
  if (c->vol.sed_alloc) return VX_OK;
  const size_t nb = c->vol.seg.nb;
  return carve(c, c->vol.sed_alloc, [&](Carve& k) {
    c->vol.sed_mask[0] = k.take<uint64_t>(nb * 8u);
    c->vol.sed_mask[1] = k.take<uint64_t>(nb * 8u);
    c->vol.sed_any = k.take<uint32_t>(nb);
  });
}

// The tail of every call that rewrites the mask outright (behind event 0 of sed_timer and the call's launches): the statistics
// of the new mask, the two times vx_segment_edit_stats reports, the result.  The flood's rounds and visits are kept when `fill`;
// `pred`: SegDev::pred now holds this mask's predicate.  Ends synchronised.
static int finish_mask_edit(VxContext* c, bool fill, bool pred, VxSegmentResult* out) {
  SegStats st;
  if (int rc = c->sed_timer.mark(c, 1)) return rc;
  if (int rc = seg_mask_stats(c, c->sed_timer, 2, &st)) return rc;
  if (int rc = c->sed_timer.read(c)) return rc;
  VxSegmentResult r = seg_result(st);
  r.rounds = fill ? st.rounds : 0u;
  r.converged = 1u;
  r.brick_visits = fill ? st.visits : 0u;
  c->vol.seg_valid = true;
  if (pred) c->vol.seg_pred_valid = true;
  if (out) *out = r;
  return VX_OK;
}

// `steps` steps of one kind from the mask at *cur.  A step never writes the mask it reads: the chain alternates between the two
// scratch masks, and the last step of the edit (`last`) writes SegDev::seg itself unless it would read it, so the masked render
// kernels, seg_pack and the overlay keep the one pointer they read at launch time.
static void launch_sed_steps(VxContext* c, int conn, bool invert, bool band, uint32_t steps, bool last, uint64_t** cur) {
  const SegDev& s = c->vol.seg;
  const uint32_t blocks = std::min<uint32_t>((s.nb + 255u) / 256u, 4096u);
  const uint64_t inv = invert ? ~0ull : 0ull;
  for (uint32_t i = 0; i < steps; ++i) {
    uint64_t* src = *cur;
    uint64_t* dst = (last && i + 1u == steps && src != s.seg) ? s.seg : (src == c->vol.sed_mask[0] ? c->vol.sed_mask[1] : c->vol.sed_mask[0]);
    with_conn(conn, [&](auto conn_c) {
      with_bool(band, [&](auto band_c) {
        hipLaunchKernelGGL((sed_step<decltype(conn_c)::value, decltype(band_c)::value>), dim3(blocks), dim3(256), 0, c->stream, src,
                           dst, s.pred, inv, s.bc[0], s.bc[1], s.bc[2]);
      });
    });
    *cur = dst;
    ++c->sed_launches;
  }
}

// ---- distances and margins (vx_segment_distance, vx_distance_read, vx_segment_margin; kernels in vx_distance.hpp) ------------
constexpr uint32_t DST_MAX_PARTIALS = 1024;

// the field (4 B per voxel) and the partials of its statistics
static int ensure_distance(VxContext* c) {
  const uint32_t* E = c->vol.dv.extent;
  if (int rc = c->vol.dist_field.ensure(c, (size_t)E[0] * E[1] * E[2])) return rc;
  return c->vol.dist_partials.ensure(c, DST_MAX_PARTIALS);
}

// the longest line the y / z passes hold in LDS (one column of it at the least)
static uint32_t dst_max_line(const VxContext* c) { return c->sw.dist_lds_bytes / 4u; }

static int check_spacing(VxContext* c, const char* fn, const float sp[3]) {
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(sp[a]) || !(sp[a] > 0.0f))
      VX_FAIL(c, VX_ERR_INVALID, "%s: spacing[%d] = %g is not finite and > 0", fn, a, (double)sp[a]);
  return VX_OK;
}
// the y and z lines of the volume fit the LDS of a line pass
static int check_line_extent(VxContext* c, const char* fn) {
  const uint32_t* E = c->vol.dv.extent;
  for (int a = 1; a < 3; ++a)
    if (E[a] > dst_max_line(c))
      VX_FAIL(c, VX_ERR_INVALID, "%s: index extent %u on axis %d is beyond the %u voxels of a line the distance passes hold in LDS", fn,
              E[a], a, dst_max_line(c));
  return VX_OK;
}

// the host's copy of dst_term (the same two fp32 products; this unit is built without contraction) and the window it gives a
// cap: the largest n <= L - 1 with term(n) <= r2.  Terms grow with n, so the first one above the cap ends the search.
static float dst_term_host(uint32_t n, float s) {
  const float p = (float)n * s;
  return p * p;
}
static uint32_t dst_window(float s, float r2, uint32_t L) {
  uint32_t w = 0;
  while (w + 1u < L && dst_term_host(w + 1u, s) <= r2) ++w;
  return w;
}

// One transform on the stream: the field = D2 of the mask `src` (complemented by inv) under the cap r2, events ev0 .. ev0 + 3 of
// dst_timer ahead of the x, y and z pass and behind the last.  The tile of a line pass is the widest of 32, 16, ... 1 columns
// whose whole lines fit the LDS budget (DESIGN.md section 2 "Distances and margins").
static int run_distance(VxContext* c, const uint64_t* src, uint64_t inv, const float sp[3], float r2, int ev0) {
  const SegDev& s = c->vol.seg;
  const uint32_t* E = c->vol.dv.extent;
  float* field = c->vol.dist_field;
  const size_t rows = (size_t)E[1] * E[2] * s.bc[0];
  if (int rc = c->dst_timer.mark(c, ev0)) return rc;
  hipLaunchKernelGGL(dst_xpass, dim3((uint32_t)std::min<size_t>((rows + 255u) / 256u, 65536u)), dim3(256), 0, c->stream, src, inv, field,
                     s.bc[0], s.bc[1], s.bc[2], sp[0], dst_window(sp[0], r2, E[0]));
  VX_HIP(c, hipGetLastError());
  for (int axis = 1; axis < 3; ++axis) {
    if (int rc = c->dst_timer.mark(c, ev0 + axis)) return rc;
    const uint32_t L = E[axis];
    uint32_t tx = 32;
    while (tx > 1u && (size_t)L * tx * 4u > c->sw.dist_lds_bytes) tx >>= 1;
    const uint32_t ntx = (E[0] + tx - 1u) / tx, nouter = axis == 1 ? E[2] : E[1];
    const size_t plane = (size_t)E[0] * E[1];
    const size_t lstride = axis == 1 ? E[0] : plane, ostride = axis == 1 ? plane : E[0];
    const uint32_t w = dst_window(sp[axis], r2, L);
    auto launch = [&](auto k) {
      hipLaunchKernelGGL((dst_linepass<decltype(k)::value>), dim3(ntx * nouter), dim3(256), (size_t)L * tx * 4u, c->stream, field, E[0], L,
                         lstride, ostride, ntx, sp[axis], w, r2);
    };
    switch (tx) {
      case 32: launch(std::integral_constant<int, 32>{}); break;
      case 16: launch(std::integral_constant<int, 16>{}); break;
      case 8: launch(std::integral_constant<int, 8>{}); break;
      case 4: launch(std::integral_constant<int, 4>{}); break;
      case 2: launch(std::integral_constant<int, 2>{}); break;
      default: launch(std::integral_constant<int, 1>{}); break;
    }
    VX_HIP(c, hipGetLastError());
  }
  c->dst_launches += 3;
  return c->dst_timer.mark(c, ev0 + 3);
}

// compare and pack behind a transform: the mask in SegDev::seg from the field (dst_pack), event ev of dst_timer behind it
static int pack_distance(VxContext* c, bool shrink, bool band, float r2, int ev) {
  const SegDev& s = c->vol.seg;
  const size_t words = (size_t)s.nb * 8u;
  hipLaunchKernelGGL(dst_pack, dim3((uint32_t)std::min<size_t>((words + 255u) / 256u, 16384u)), dim3(256), 0, c->stream,
                     (const float*)c->vol.dist_field, s.seg, band ? (const uint64_t*)s.pred : nullptr, shrink ? 1u : 0u, s.bc[0], s.bc[1],
                     s.bc[2], r2);
  VX_HIP(c, hipGetLastError());
  ++c->dst_launches;
  return c->dst_timer.mark(c, ev);
}

// the unused events of dst_timer from `from` to `to`, back to back (read() takes every pair)
static int mark_rest(VxContext* c, int from, int to) {
  for (int i = from; i <= to; ++i)
    if (int rc = c->dst_timer.mark(c, i)) return rc;
  return VX_OK;
}
// the times of `rounds` transforms (4 stages each from event 0), summed per pass; every event is recorded and complete
static int read_distance_times(VxContext* c, int rounds) {
  if (int rc = c->dst_timer.read(c)) return rc;
  for (int k = 0; k < 4; ++k) c->dst_ms[k] = c->dst_timer.ms[k] + (rounds > 1 ? c->dst_timer.ms[4 + k] : 0.0);
  return VX_OK;
}

// ---- the segment store (vx_segment_store .. vx_segments_labelmap; kernels in vx_segstore.hpp) ----------------------------------
constexpr uint32_t SST_MAX_PARTIALS = 1024;

// `slot` names a slot; with `occupied`, one that holds a mask
static int check_slot(VxContext* c, const char* fn, uint32_t slot, bool occupied) {
  if (slot >= VX_SEGMENT_SLOTS) VX_FAIL(c, VX_ERR_INVALID, "%s: slot = %u outside 0 .. %u", fn, slot, VX_SEGMENT_SLOTS - 1u);
  if (occupied && !c->vol.slots[slot].p)
    VX_FAIL(c, VX_ERR_INVALID, "%s: slot %u is empty (vx_segment_store first; vx_segment_drop and an upload empty it)", fn, slot);
  return VX_OK;
}
static int check_current(VxContext* c, const char* fn) {
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "%s: no current segment (vx_segment, vx_segment_threshold, vx_segment_write_mask or vx_segment_load "
                               "first; an upload drops it)", fn);
  return VX_OK;
}

// behind an uncapped transform: the largest D2 over the voxels of `over` into partials[0] (sst_max_over, dst_reduce_final)
static int launch_max_over(VxContext* c, const uint64_t* over, DstPartial* partials) {
  const SegDev& s = c->vol.seg;
  const size_t words = (size_t)s.nb * 8u;
  const uint32_t blocks = (uint32_t)std::min<size_t>((words + 255u) / 256u, DST_MAX_PARTIALS / 2u);
  hipLaunchKernelGGL(sst_max_over, dim3(blocks), dim3(256), 0, c->stream, (const float*)c->vol.dist_field, over, s.bc[0], s.bc[1], s.bc[2],
                     partials);
  hipLaunchKernelGGL(dst_reduce_final, dim3(1), dim3(256), 0, c->stream, partials, blocks);
  VX_HIP(c, hipGetLastError());
  c->dst_launches += 2;
  return VX_OK;
}

// ---- histograms (vx_histogram; kernels in vx_histogram.hpp) ------------------------------------------------------------------------
// hst_bins for the resident layout and the two wave-uniform choices of the call
static void launch_hst_bins(VxContext* c, const HstParams& h, bool moments, uint32_t blocks) {
  const VxParams& p = c->params;
  with_layout(slice_layout(c), [&](auto lay) {
    with_bool(h.mask != nullptr, [&](auto masked) {
      with_bool(moments, [&](auto mom) {
        hipLaunchKernelGGL((hst_bins<decltype(lay)::value, decltype(masked)::value, decltype(mom)::value>), dim3(blocks), dim3(256), 0,
                           c->stream, c->vol.dv, p.volume_density_scale, p.volume_inv_maj, h);
      });
    });
  });
}

static int ensure_islands(VxContext* c) {
  if (c->vol.isl_alloc) return VX_OK;
  const size_t nb = c->vol.seg.nb;
  IslDev& d = c->vol.isl;
  return carve(c, c->vol.isl_alloc, [&](Carve& k) {
    d.lab = k.take<uint32_t>(nb * 512u);
    d.nroots = k.take<uint32_t>(nb);
    d.off = k.take<uint32_t>(nb);
    d.hdr = k.take<IslHdr>();
  });
}

// room for n rows and their labels, 1024 at least (every earlier call has completed: each one synchronises)
static int ensure_island_rows(VxContext* c, uint32_t n) {
  IslDev& d = c->vol.isl;
  n = std::max(n, 1u);
  if (n <= d.cap) return VX_OK;
  d.cap = 0;
  const size_t cap = std::max<size_t>(n, 1024u);
  const int rc = carve(c, c->vol.isl_rows_alloc, [&](Carve& k) {
    d.rows = k.take<IslRow>(cap);
    d.newlab = k.take<uint32_t>(cap);
  });
  if (rc) return rc;
  d.cap = (uint32_t)cap;
  return VX_OK;
}

}  // namespace

extern "C" {

int vx_segment(VxContext* c, const VxSegmentParams* sp, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment(c->members[0], sp, out));
  VX_DEV(c);
  VoxelBox box;
  if (int rc = check_ready(c, "vx_segment", sp, "sp")) return rc;
  if (int rc = check_seed(c, "vx_segment", sp->seed)) return rc;
  if (int rc = check_band(c, "vx_segment", sp->lo, sp->hi)) return rc;
  if (int rc = check_connectivity(c, "vx_segment", sp->connectivity)) return rc;
  if (int rc = check_box(c, "vx_segment", sp->box_lo, sp->box_hi, &box)) return rc;
  c->vol.seg_valid = false;
  c->vol.seg_pred_valid = false;
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  if (int rc = ensure_segment(c)) return rc;
  const SegDev& s = c->vol.seg;
  const uint32_t* E = c->vol.dv.extent;
  const SegSeed seed = seg_seed_of(s, sp->seed);
  const uint64_t nvox = (uint64_t)E[0] * E[1] * E[2];
  const uint64_t cap = sp->max_rounds ? (uint64_t)sp->max_rounds : std::min<uint64_t>(nvox, 0xfffffffeull);
  VX_HIP(c, hipMemsetAsync(s.seg, 0, (size_t)s.nb * 64u, c->stream));
  VX_HIP(c, hipMemsetAsync(s.stamp, 0, (size_t)s.nb * 4u, c->stream));
  if (int rc = c->seg_timer.mark(c, 0)) return rc;
  launch_seg_predicate(c, seg_pred_params(sp->lo, sp->hi, box));
  VX_HIP(c, hipGetLastError());
  if (int rc = c->seg_timer.mark(c, 1)) return rc;
  hipLaunchKernelGGL(seg_seed, dim3(1), dim3(64), 0, c->stream, s, seed);
  VX_HIP(c, hipGetLastError());
  bool converged = false;
  if (int rc = run_seg_flood(c, s, sp->connectivity, seed, cap, &converged, nullptr)) return rc;
  if (int rc = c->seg_timer.mark(c, 2)) return rc;
  launch_seg_stats(c);
  VX_HIP(c, hipGetLastError());
  if (int rc = c->seg_timer.mark(c, 3)) return rc;
  SegStats st;
  VX_HIP(c, hipMemcpyAsync(&st, s.st, sizeof st, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->seg_timer.read(c)) return rc;
  VxSegmentResult r = seg_result(st);
  r.rounds = st.rounds;
  r.converged = converged ? 1u : 0u;
  r.brick_visits = st.visits;
  c->seg_res = r;
  c->vol.seg_valid = true;
  c->vol.seg_pred_valid = true;
  if (out) *out = r;
  return VX_OK;
}

int vx_segment_read_mask(VxContext* c, uint8_t* bits, uint64_t nbytes) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_read_mask(c->members[0], bits, nbytes));
  VX_DEV(c);
  if (!c->vol.seg_valid) VX_FAIL(c, VX_ERR_INVALID, "vx_segment_read_mask: no current segment (vx_segment first; an upload drops it)");
  if (!bits) VX_FAIL(c, VX_ERR_INVALID, "vx_segment_read_mask: bits is NULL");
  const uint32_t* E = c->vol.dv.extent;
  size_t want = 0;
  if (int rc = check_mask_bytes(c, "vx_segment_read_mask", nbytes, &want)) return rc;
  if (int rc = c->vol.seg_bytes.ensure(c, want)) return rc;   // (every earlier call has completed: each one synchronises)
  const uint32_t blocks = (uint32_t)std::min<size_t>((want + 255u) / 256u, 8192u);
  hipLaunchKernelGGL(seg_pack, dim3(blocks), dim3(256), 0, c->stream, c->vol.seg, E[0], E[1], want, c->vol.seg_bytes);
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipMemcpyAsync(bits, c->vol.seg_bytes, want, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_slice_segment_mask(VxContext* c, const VxSliceParams* sp, uint8_t* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_slice_segment_mask(c->members[0], sp, out));
  VX_DEV(c);
  if (!c->vol.has_volume) VX_FAIL(c, VX_ERR_NO_VOLUME, "vx_slice_segment_mask: no volume uploaded");
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_slice_segment_mask: no current segment (vx_segment first; an upload drops it)");
  if (!sp) VX_FAIL(c, VX_ERR_INVALID, "vx_slice_segment_mask: sp is NULL");
  if (!out) VX_FAIL(c, VX_ERR_INVALID, "vx_slice_segment_mask: out is NULL");
  if (int rc = check_slice_size(c, "vx_slice_segment_mask", sp)) return rc;
  if (int rc = check_slice_frame(c, "vx_slice_segment_mask", sp)) return rc;
  const size_t px = (size_t)sp->size[0] * sp->size[1];
  if (int rc = c->seg_ov.ensure(c, px)) return rc;   // (every earlier call has completed: each one synchronises)
  const dim3 grid((sp->size[0] + 15u) / 16u, (sp->size[1] + 15u) / 16u);
  hipLaunchKernelGGL(seg_slice_mask, grid, dim3(256), 0, c->stream, *sp, c->vol.seg, c->vol.dv.extent[0], c->vol.dv.extent[1],
                     c->vol.dv.extent[2], c->seg_ov);
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipMemcpyAsync(out, c->seg_ov, px, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_set_segment_view(VxContext* c, int view) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return refuse_group(c, "vx_set_segment_view", "the segment lives on member 0 only");
  if (view < VX_SEGVIEW_OFF || view > VX_SEGVIEW_HIDE)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_segment_view: view = %d is not VX_SEGVIEW_OFF, _ONLY or _HIDE", view);
  if (view != VX_SEGVIEW_OFF && !c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_segment_view: %s without a current segment (vx_segment first; an upload drops it)",
            view == VX_SEGVIEW_ONLY ? "only" : "hide");
  c->vol.seg_view = view;
  return VX_OK;
}

int vx_get_segment_view(VxContext* c, int* view) {
  if (!c || !view) return VX_ERR_INVALID;
  *view = c->vol.seg_view;
  return VX_OK;
}

int vx_segment_stats(VxContext* c, uint32_t* rounds, uint64_t* brick_visits, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_stats(c->members[0], rounds, brick_visits, kernel_ms));
  if (rounds) *rounds = c->seg_res.rounds;
  if (brick_visits) *brick_visits = c->seg_res.brick_visits;
  if (kernel_ms) std::copy_n(c->seg_timer.ms, 3, kernel_ms);
  return VX_OK;
}

int vx_segment_edit(VxContext* c, const VxSegmentEditParams* ep, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_edit(c->members[0], ep, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_edit", ep, "params")) return rc;
  if (ep->op < VX_SEGEDIT_DILATE || ep->op > VX_SEGEDIT_FILL_HOLES)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: op = %d is not a VxSegmentEditOp (0 .. 4)", ep->op);
  if (int rc = check_connectivity(c, "vx_segment_edit", ep->connectivity)) return rc;
  const bool fill = ep->op == VX_SEGEDIT_FILL_HOLES;
  if (fill ? ep->steps > 1u : (ep->steps < 1u || ep->steps > VX_SEGEDIT_MAX_STEPS))
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: steps = %u outside %s", ep->steps, fill ? "0 .. 1 (fill holes)" : "1 .. 1024");
  if (ep->band != 0 && ep->band != 1) VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: band = %d is not 0 or 1", ep->band);
  if (ep->band && ep->op != VX_SEGEDIT_DILATE)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: band = 1 is for VX_SEGEDIT_DILATE only (op = %d)", ep->op);
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: no current segment (vx_segment or vx_segment_write_mask first; an upload drops it)");
  if (ep->band && !c->vol.seg_pred_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_edit: band = 1 without a predicate on this volume (vx_segment first; an upload drops it)");
  if (int rc = ensure_segedit(c)) return rc;
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  const int conn = ep->connectivity;
  const uint32_t n = ep->steps;
  c->sed_launches = 0;
  if (int rc = c->sed_timer.mark(c, 0)) return rc;
  uint64_t* cur = s.seg;
  switch (ep->op) {
    case VX_SEGEDIT_DILATE: launch_sed_steps(c, conn, false, ep->band != 0, n, true, &cur); break;
    case VX_SEGEDIT_ERODE: launch_sed_steps(c, conn, true, false, n, true, &cur); break;
    case VX_SEGEDIT_OPEN:
      launch_sed_steps(c, conn, true, false, n, false, &cur);
      launch_sed_steps(c, conn, false, false, n, true, &cur);
      break;
    case VX_SEGEDIT_CLOSE:
      launch_sed_steps(c, conn, false, false, n, false, &cur);
      launch_sed_steps(c, conn, true, false, n, true, &cur);
      break;
    default: {
      // the background flood on a second view: predicate ~M and the reached set in the scratch masks, the bookkeeping shared
      // with vx_segment (its predicate WORDS stay: band dilation after a fill is legal)
      SegDev f = s;
      f.pred = c->vol.sed_mask[0];
      f.seg = c->vol.sed_mask[1];
      f.any = c->vol.sed_any;
      const uint32_t blocks = std::min<uint32_t>((s.nb + 255u) / 256u, 4096u);
      hipLaunchKernelGGL(sed_reset, dim3(1), dim3(64), 0, c->stream, s, 1u);
      hipLaunchKernelGGL(sed_fill_seed, dim3(blocks), dim3(256), 0, c->stream, s.seg, f);
      VX_HIP(c, hipGetLastError());
      bool converged = false;
      uint64_t launched = 0;
      const uint64_t nvox = (uint64_t)c->vol.dv.extent[0] * c->vol.dv.extent[1] * c->vol.dv.extent[2];
      if (int rc = run_seg_flood(c, f, conn, SegSeed{0u, 0u, 0ull}, std::min<uint64_t>(nvox, 0xfffffffeull), &converged, &launched))
        return rc;
      const size_t words = (size_t)s.nb * 8u;
      hipLaunchKernelGGL(sed_fill_finish, dim3((uint32_t)std::min<size_t>((words + 255u) / 256u, 8192u)), dim3(256), 0, c->stream,
                         f.seg, s.seg, words);
      c->sed_launches = (uint32_t)std::min<uint64_t>(launched + 3u, 0xffffffffull);
      cur = s.seg;
    }
  }
  VX_HIP(c, hipGetLastError());
  // a single step read SegDev::seg and so wrote a scratch mask: copy it home on the stream
  if (cur != s.seg) VX_HIP(c, hipMemcpyAsync(s.seg, cur, (size_t)s.nb * 64u, hipMemcpyDeviceToDevice, c->stream));
  return finish_mask_edit(c, fill, false, out);
}

int vx_segment_write_mask(VxContext* c, const uint8_t* bits, uint64_t nbytes, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_write_mask(c->members[0], bits, nbytes, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_write_mask", bits, "bits")) return rc;
  size_t want = 0;
  if (int rc = check_mask_bytes(c, "vx_segment_write_mask", nbytes, &want)) return rc;
  if (int rc = ensure_segment(c)) return rc;
  if (int rc = ensure_segedit(c)) return rc;
  if (int rc = c->vol.seg_bytes.ensure(c, want)) return rc;   // (every earlier call has completed: each one synchronises)
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  VX_HIP(c, hipMemcpyAsync(c->vol.seg_bytes, bits, want, hipMemcpyHostToDevice, c->stream));
  if (int rc = c->sed_timer.mark(c, 0)) return rc;
  const size_t words = (size_t)s.nb * 8u;
  hipLaunchKernelGGL(sed_unpack, dim3((uint32_t)std::min<size_t>((words + 255u) / 256u, 8192u)), dim3(256), 0, c->stream, s,
                     c->vol.dv.extent[1], c->vol.seg_bytes);
  VX_HIP(c, hipGetLastError());
  c->sed_launches = 1;
  return finish_mask_edit(c, false, false, out);
}

int vx_segment_edit_stats(VxContext* c, uint32_t* launches, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_edit_stats(c->members[0], launches, kernel_ms));
  if (launches) *launches = c->sed_launches;
  if (kernel_ms) std::copy_n(c->sed_timer.ms, 2, kernel_ms);
  return VX_OK;
}

// ---- islands (vx_segment_threshold, vx_segment_islands, vx_islands_read*; kernels in vx_islands.hpp) ---------------------------
// (the mask is rewritten outright: timed and counted like vx_segment_write_mask, reported by vx_segment_edit_stats)
int vx_segment_threshold(VxContext* c, const VxSegmentParams* sp, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_threshold(c->members[0], sp, out));
  VX_DEV(c);
  VoxelBox box;
  if (int rc = check_ready(c, "vx_segment_threshold", sp, "sp")) return rc;
  if (int rc = check_band(c, "vx_segment_threshold", sp->lo, sp->hi)) return rc;
  if (int rc = check_box(c, "vx_segment_threshold", sp->box_lo, sp->box_hi, &box)) return rc;
  if (int rc = ensure_segment(c)) return rc;
  c->vol.seg_valid = false;
  c->vol.seg_pred_valid = false;
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  if (int rc = c->sed_timer.mark(c, 0)) return rc;
  launch_seg_predicate(c, seg_pred_params(sp->lo, sp->hi, box));
  VX_HIP(c, hipGetLastError());
  // the mask = the predicate words.  SegDev::seg keeps its address: the masked render kernels read it at launch time
  VX_HIP(c, hipMemcpyAsync(s.seg, s.pred, (size_t)s.nb * 64u, hipMemcpyDeviceToDevice, c->stream));
  c->sed_launches = 1;
  return finish_mask_edit(c, false, true, out);
}

int vx_segment_islands(VxContext* c, const VxIslandsParams* ip, VxIslandsResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_islands(c->members[0], ip, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_islands", ip, "params")) return rc;
  if (ip->op < VX_ISLANDS_LABEL || ip->op > VX_ISLANDS_KEEP_AT)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_islands: op = %d is not a VxIslandsOp (0 .. 3)", ip->op);
  if (int rc = check_connectivity(c, "vx_segment_islands", ip->connectivity)) return rc;
  if (ip->op == VX_ISLANDS_KEEP_LARGEST && ip->keep == 0)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_islands: keep = 0 (KEEP_LARGEST keeps at least one island)");
  if (ip->op == VX_ISLANDS_REMOVE_SMALL && ip->min_voxels == 0)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_islands: min_voxels = 0 (REMOVE_SMALL needs a size of at least 1)");
  const uint32_t* E = c->vol.dv.extent;
  if (ip->op == VX_ISLANDS_KEEP_AT)
    if (int rc = check_seed(c, "vx_segment_islands", ip->seed)) return rc;
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_islands: no current segment (vx_segment, vx_segment_threshold or vx_segment_write_mask "
                               "first; an upload drops it)");
  const uint64_t nvox = (uint64_t)E[0] * E[1] * E[2];
  if (nvox >= 0x80000000ull)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_islands: %llu voxels are beyond the 31-bit voxel index of the labels",
            (unsigned long long)nvox);
  if (int rc = ensure_islands(c)) return rc;
  if (int rc = ensure_island_rows(c, 1u)) return rc;
  c->vol.isl_valid = false;
  const SegDev& s = c->vol.seg;
  const bool modify = ip->op != VX_ISLANDS_LABEL;
  if (modify) c->vol.dist_valid = false;
  const dim3 grid(std::min<uint32_t>((s.nb + 3u) / 4u, 16384u)), block(256);
  uint32_t launches = 0;
  VX_HIP(c, hipMemsetAsync(c->vol.isl.hdr, 0, sizeof(IslHdr), c->stream));
  StageTimer<7>& timer = c->isl_timer;
  if (int rc = timer.mark(c, 0)) return rc;
  with_conn(ip->connectivity, [&](auto k) { hipLaunchKernelGGL(isl_local<decltype(k)::value>, grid, block, 0, c->stream, s, c->vol.isl); });
  if (int rc = timer.mark(c, 1)) return rc;
  with_conn(ip->connectivity, [&](auto k) { hipLaunchKernelGGL(isl_merge<decltype(k)::value>, grid, block, 0, c->stream, s, c->vol.isl); });
  if (int rc = timer.mark(c, 2)) return rc;
  hipLaunchKernelGGL(isl_flatten, grid, block, 0, c->stream, s, c->vol.isl);
  hipLaunchKernelGGL(isl_scan, dim3(1), dim3(1024), 0, c->stream, s, c->vol.isl);
  VX_HIP(c, hipGetLastError());
  launches += 4;
  if (int rc = timer.mark(c, 3)) return rc;
  // the one read-back that sizes the table: the number of islands
  IslHdr hdr{};
  VX_HIP(c, hipMemcpyAsync(&hdr, c->vol.isl.hdr, sizeof hdr, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  const uint32_t R = hdr.roots;
  if (int rc = ensure_island_rows(c, R)) return rc;
  const IslDev& d = c->vol.isl;
  const SegSeed seed = ip->op == VX_ISLANDS_KEEP_AT ? seg_seed_of(s, ip->seed) : SegSeed{0u, 0u, 1ull};
  hipLaunchKernelGGL(isl_rootid, grid, block, 0, c->stream, s, d);
  hipLaunchKernelGGL(isl_table, grid, block, 0, c->stream, s, d);
  hipLaunchKernelGGL(isl_seed_row, dim3(1), dim3(64), 0, c->stream, s, d, seed);
  VX_HIP(c, hipGetLastError());
  launches += 3;
  if (int rc = timer.mark(c, 4)) return rc;
  VX_HIP(c, hipEventSynchronize(timer.ev[4]));
  // the host's share: the rows come back once, are ranked by (count descending, anchor ascending), and every row's label
  // (0: dropped by the op) goes back up.  O(islands), not O(voxels).
  const auto t0 = std::chrono::steady_clock::now();
  std::vector<IslRow> rows(R);
  VX_HIP(c, hipMemcpyAsync(&hdr, d.hdr, sizeof hdr, hipMemcpyDeviceToHost, c->stream));
  if (R) VX_HIP(c, hipMemcpyAsync(rows.data(), d.rows, (size_t)R * sizeof(IslRow), hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  std::vector<uint32_t> order(R);
  for (uint32_t i = 0; i < R; ++i) order[i] = i;
  std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) {
    return rows[a].count != rows[b].count ? rows[a].count > rows[b].count : rows[a].anchor < rows[b].anchor;
  });
  std::vector<uint32_t> newlab(std::max(R, 1u), 0u);
  std::vector<VxIsland> table;
  table.reserve(R);
  for (uint32_t k = 0; k < R; ++k) {
    const uint32_t i = order[k];
    const IslRow& r = rows[i];
    bool keep = true;
    switch (ip->op) {
      case VX_ISLANDS_KEEP_LARGEST: keep = (uint64_t)k < ip->keep; break;
      case VX_ISLANDS_REMOVE_SMALL: keep = r.count >= ip->min_voxels; break;
      case VX_ISLANDS_KEEP_AT: keep = i == hdr.seed_row; break;
      default: break;
    }
    if (!keep) continue;
    VxIsland v{};
    v.count = r.count;
    v.anchor[0] = r.anchor % E[0];
    v.anchor[1] = (r.anchor / E[0]) % E[1];
    v.anchor[2] = r.anchor / (E[0] * E[1]);
    for (int a = 0; a < 3; ++a) {
      v.bbox_lo[a] = r.lo[a];
      v.bbox_hi[a] = r.hi[a];
    }
    table.push_back(v);
    table.back().label = (uint32_t)table.size();
    newlab[i] = (uint32_t)table.size();
  }
  VX_HIP(c, hipMemcpyAsync(d.newlab, newlab.data(), newlab.size() * 4u, hipMemcpyHostToDevice, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));   // (newlab is pageable host memory of this frame)
  const double host_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (int rc = timer.mark(c, 5)) return rc;
  if (modify) {
    hipLaunchKernelGGL(isl_apply, grid, block, 0, c->stream, s, d);
    ++launches;
  }
  if (int rc = timer.mark(c, 6)) return rc;
  SegStats st;
  if (int rc = seg_mask_stats(c, timer, 7, &st)) return rc;
  launches += 3;
  if (int rc = timer.read(c)) return rc;
  timer.ms[4] = host_ms;             // stage 4 is the host's share: wall time, not the events around it
  if (!modify) timer.ms[5] = 0.0;    // (two events back to back still measure a few microseconds)
  c->isl_launches = launches;
  VxIslandsResult r{};
  r.islands = R;
  r.kept = table.size();
  r.largest = R ? rows[order[0]].count : 0u;
  r.seg = seg_result(st);
  r.seg.converged = 1u;
  c->vol.isl_table.swap(table);
  c->vol.isl_valid = true;
  if (out) *out = r;
  return VX_OK;
}

int vx_islands_read(VxContext* c, uint64_t first, uint64_t n, VxIsland* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_islands_read(c->members[0], first, n, out));
  if (!c->vol.isl_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read: no current table (vx_segment_islands first; an upload and every call that "
                               "changes the segment drop it)");
  const uint64_t have = c->vol.isl_table.size();
  if (first > have || n > have - first)
    VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read: rows %llu .. %llu are beyond the %llu islands of the table",
            (unsigned long long)first, (unsigned long long)(first + n), (unsigned long long)have);
  if (n && !out) VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read: out is NULL");
  if (n) memcpy(out, c->vol.isl_table.data() + first, (size_t)n * sizeof(VxIsland));
  return VX_OK;
}

int vx_islands_read_labels(VxContext* c, uint32_t* labels, uint64_t nvoxels) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_islands_read_labels(c->members[0], labels, nvoxels));
  VX_DEV(c);
  if (!c->vol.isl_valid || !c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read_labels: no current table (vx_segment_islands first; an upload and every call "
                               "that changes the segment drop it)");
  if (!labels) VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read_labels: labels is NULL");
  const uint32_t* E = c->vol.dv.extent;
  const size_t want = (size_t)E[0] * E[1] * E[2];
  if (nvoxels != want)
    VX_FAIL(c, VX_ERR_INVALID, "vx_islands_read_labels: nvoxels = %llu, the volume has %u x %u x %u = %zu voxels",
            (unsigned long long)nvoxels, E[0], E[1], E[2], want);
  if (int rc = c->vol.isl_dense.ensure(c, want)) return rc;   // (every earlier call has completed: each one synchronises)
  const uint32_t blocks = (uint32_t)std::min<size_t>((want + 255u) / 256u, 16384u);
  hipLaunchKernelGGL(isl_labels_out, dim3(blocks), dim3(256), 0, c->stream, c->vol.seg, c->vol.isl, E[0], E[1], want, c->vol.isl_dense);
  VX_HIP(c, hipGetLastError());
  VX_HIP(c, hipMemcpyAsync(labels, c->vol.isl_dense, want * 4u, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_islands_stats(VxContext* c, uint32_t* launches, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_islands_stats(c->members[0], launches, kernel_ms));
  if (launches) *launches = c->isl_launches;
  if (kernel_ms) std::copy_n(c->isl_timer.ms, 7, kernel_ms);
  return VX_OK;
}

// ---- distances and margins -------------------------------------------------------------------------------------------------------
int vx_segment_distance(VxContext* c, const VxDistanceParams* dp, VxDistanceResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_distance(c->members[0], dp, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_distance", dp, "params")) return rc;
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_distance: no current segment (vx_segment, vx_segment_threshold or vx_segment_write_mask "
                               "first; an upload drops it)");
  if (int rc = check_spacing(c, "vx_segment_distance", dp->spacing)) return rc;
  if (int rc = check_line_extent(c, "vx_segment_distance")) return rc;
  if (!(dp->max_distance > 0.0f))
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_distance: max_distance = %g is not > 0 (+inf: no cap)", (double)dp->max_distance);
  if (dp->side != VX_DISTANCE_OUTSIDE && dp->side != VX_DISTANCE_INSIDE)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_distance: side = %d is not VX_DISTANCE_OUTSIDE or _INSIDE", dp->side);
  if (int rc = ensure_distance(c)) return rc;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  const uint32_t* E = c->vol.dv.extent;
  const float r2 = dp->max_distance * dp->max_distance;
  const uint64_t inv = dp->side == VX_DISTANCE_INSIDE ? ~0ull : 0ull;
  c->dst_launches = 0;
  if (int rc = run_distance(c, s.seg, inv, dp->spacing, r2, 0)) return rc;
  const size_t words = (size_t)s.nb * 8u;
  const uint32_t blocks = (uint32_t)std::min<size_t>((words + 255u) / 256u, DST_MAX_PARTIALS);
  DstPartial* partials = c->vol.dist_partials;
  hipLaunchKernelGGL(dst_reduce, dim3(blocks), dim3(256), 0, c->stream, (const float*)c->vol.dist_field, (const uint64_t*)s.seg, inv,
                     s.bc[0], s.bc[1], s.bc[2], r2, partials);
  hipLaunchKernelGGL(dst_reduce_final, dim3(1), dim3(256), 0, c->stream, partials, blocks);
  VX_HIP(c, hipGetLastError());
  c->dst_launches += 2;
  if (int rc = mark_rest(c, 4, 9)) return rc;
  DstPartial top{};
  VX_HIP(c, hipMemcpyAsync(&top, partials, sizeof top, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = read_distance_times(c, 1)) return rc;
  VxDistanceResult r{};
  r.finite = top.finite;
  if (top.idx != DST_NONE) {
    r.max_d2 = top.d2;
    r.argmax[0] = (uint32_t)(top.idx % E[0]);
    r.argmax[1] = (uint32_t)((top.idx / E[0]) % E[1]);
    r.argmax[2] = (uint32_t)(top.idx / ((uint64_t)E[0] * E[1]));
  }
  c->vol.dist_valid = true;
  if (out) *out = r;
  return VX_OK;
}

int vx_distance_read(VxContext* c, float* d2, uint64_t nvoxels) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_distance_read(c->members[0], d2, nvoxels));
  VX_DEV(c);
  if (!c->vol.dist_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_distance_read: no current field (vx_segment_distance first; an upload and every call that changes "
                               "or replaces the segment drop it)");
  if (!d2) VX_FAIL(c, VX_ERR_INVALID, "vx_distance_read: d2 is NULL");
  const uint32_t* E = c->vol.dv.extent;
  const size_t want = (size_t)E[0] * E[1] * E[2];
  if (nvoxels != want)
    VX_FAIL(c, VX_ERR_INVALID, "vx_distance_read: nvoxels = %llu, the volume has %u x %u x %u = %zu voxels", (unsigned long long)nvoxels,
            E[0], E[1], E[2], want);
  VX_HIP(c, hipMemcpyAsync(d2, c->vol.dist_field, want * 4u, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

int vx_segment_margin(VxContext* c, const VxMarginParams* mp, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_margin(c->members[0], mp, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_margin", mp, "params")) return rc;
  if (!c->vol.seg_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: no current segment (vx_segment, vx_segment_threshold or vx_segment_write_mask "
                               "first; an upload drops it)");
  if (int rc = check_spacing(c, "vx_segment_margin", mp->spacing)) return rc;
  if (int rc = check_line_extent(c, "vx_segment_margin")) return rc;
  if (!std::isfinite(mp->radius) || !(mp->radius > 0.0f))
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: radius = %g is not finite and > 0", (double)mp->radius);
  if (mp->op < VX_MARGIN_GROW || mp->op > VX_MARGIN_CLOSE)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: op = %d is not a VxMarginOp (0 .. 3)", mp->op);
  if (mp->band != 0 && mp->band != 1) VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: band = %d is not 0 or 1", mp->band);
  if (mp->band && mp->op != VX_MARGIN_GROW)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: band = 1 is for VX_MARGIN_GROW only (op = %d)", mp->op);
  if (mp->band && !c->vol.seg_pred_valid)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_margin: band = 1 without a predicate on this volume (vx_segment first; an upload drops it)");
  if (int rc = ensure_distance(c)) return rc;
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  const float r2 = mp->radius * mp->radius;
  // the halves of the op in order: grow measures from the segment, shrink from its complement; each packs SegDev::seg in place
  const bool first_shrinks = mp->op == VX_MARGIN_SHRINK || mp->op == VX_MARGIN_OPEN;
  const int rounds = mp->op == VX_MARGIN_OPEN || mp->op == VX_MARGIN_CLOSE ? 2 : 1;
  c->dst_launches = 0;
  // (event 4 is recorded twice with two rounds, behind the first pack and again ahead of the second x pass: adjacent on the
  // stream, and the later record is the one both neighbouring stages are read against)
  for (int k = 0; k < rounds; ++k) {
    const bool shrink = first_shrinks == (k == 0);
    if (int rc = run_distance(c, s.seg, shrink ? ~0ull : 0ull, mp->spacing, r2, 4 * k)) return rc;
    if (int rc = pack_distance(c, shrink, mp->band != 0, r2, 4 * k + 4)) return rc;
  }
  if (int rc = mark_rest(c, 4 * rounds + 1, 8)) return rc;
  SegStats st;
  if (int rc = seg_mask_stats(c, c->dst_timer, 9, &st)) return rc;
  if (int rc = read_distance_times(c, rounds)) return rc;
  VxSegmentResult r = seg_result(st);
  r.converged = 1u;
  if (out) *out = r;
  return VX_OK;
}

int vx_distance_stats(VxContext* c, uint32_t* launches, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_distance_stats(c->members[0], launches, kernel_ms));
  if (launches) *launches = c->dst_launches;
  if (kernel_ms) std::copy_n(c->dst_ms, 4, kernel_ms);
  return VX_OK;
}

// ---- the segment store -----------------------------------------------------------------------------------------------------------
// (a slot is freed or first allocated between calls: every earlier call has completed, each one synchronises)
int vx_segment_store(VxContext* c, uint32_t slot) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_store(c->members[0], slot));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_store", c, "ctx")) return rc;
  if (int rc = check_slot(c, "vx_segment_store", slot, false)) return rc;
  if (int rc = check_current(c, "vx_segment_store")) return rc;
  const SegDev& s = c->vol.seg;
  DevBuf<uint64_t>& dst = c->vol.slots[slot];
  if (!dst.p)
    if (int rc = dst.alloc(c, (size_t)s.nb * 8u)) return rc;
  VX_HIP(c, hipMemcpyAsync(dst.p, s.seg, (size_t)s.nb * 64u, hipMemcpyDeviceToDevice, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  return VX_OK;
}

// (the mask is rewritten outright: timed and counted like vx_segment_write_mask, the copy as its one launch)
int vx_segment_load(VxContext* c, uint32_t slot, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_load(c->members[0], slot, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_load", c, "ctx")) return rc;
  if (int rc = check_slot(c, "vx_segment_load", slot, true)) return rc;
  if (int rc = ensure_segment(c)) return rc;   // (there already: a slot was stored from it)
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  if (int rc = c->sed_timer.mark(c, 0)) return rc;
  // SegDev::seg keeps its address: the masked render kernels read it at launch time
  VX_HIP(c, hipMemcpyAsync(s.seg, c->vol.slots[slot].p, (size_t)s.nb * 64u, hipMemcpyDeviceToDevice, c->stream));
  c->sed_launches = 1;
  return finish_mask_edit(c, false, false, out);
}

int vx_segment_drop(VxContext* c, uint32_t slot) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_drop(c->members[0], slot));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_drop", c, "ctx")) return rc;
  if (int rc = check_slot(c, "vx_segment_drop", slot, false)) return rc;
  c->vol.slots[slot].reset();
  return VX_OK;
}

int vx_segment_slots(VxContext* c, uint32_t* occupied) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_slots(c->members[0], occupied));
  if (int rc = check_ready(c, "vx_segment_slots", occupied, "occupied")) return rc;
  uint32_t bits = 0;
  for (uint32_t k = 0; k < VX_SEGMENT_SLOTS; ++k)
    if (c->vol.slots[k].p) bits |= 1u << k;
  *occupied = bits;
  return VX_OK;
}

int vx_segment_combine(VxContext* c, const VxCombineParams* cp, VxSegmentResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_combine(c->members[0], cp, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_combine", cp, "params")) return rc;
  if (cp->op < VX_COMBINE_UNION || cp->op > VX_COMBINE_INVERT)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_combine: op = %d is not a VxCombineOp (0 .. 4)", cp->op);
  const bool invert = cp->op == VX_COMBINE_INVERT;
  if (!invert)
    if (int rc = check_slot(c, "vx_segment_combine", cp->slot, false)) return rc;
  if (int rc = check_current(c, "vx_segment_combine")) return rc;
  if (!invert)
    if (int rc = check_slot(c, "vx_segment_combine", cp->slot, true)) return rc;
  c->vol.isl_valid = false;
  c->vol.dist_valid = false;
  const SegDev& s = c->vol.seg;
  if (int rc = c->sed_timer.mark(c, 0)) return rc;
  const size_t pairs = (size_t)s.nb * 4u;
  hipLaunchKernelGGL(sst_combine, dim3((uint32_t)std::min<size_t>((pairs + 255u) / 256u, 8192u)), dim3(256), 0, c->stream, s.seg,
                     invert ? (const uint64_t*)nullptr : (const uint64_t*)c->vol.slots[cp->slot].p, cp->op, pairs);
  VX_HIP(c, hipGetLastError());
  c->sed_launches = 1;
  return finish_mask_edit(c, false, false, out);
}

int vx_segment_compare(VxContext* c, const VxCompareParams* cp, VxCompareResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segment_compare(c->members[0], cp, out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segment_compare", cp, "params")) return rc;
  if (int rc = check_slot(c, "vx_segment_compare", cp->slot, false)) return rc;
  if (int rc = check_current(c, "vx_segment_compare")) return rc;
  if (int rc = check_slot(c, "vx_segment_compare", cp->slot, true)) return rc;
  if (cp->hausdorff != 0 && cp->hausdorff != 1)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segment_compare: hausdorff = %d is not 0 or 1", cp->hausdorff);
  if (cp->hausdorff) {
    if (int rc = check_spacing(c, "vx_segment_compare", cp->spacing)) return rc;
    if (int rc = check_line_extent(c, "vx_segment_compare")) return rc;
    if (int rc = ensure_distance(c)) return rc;
  }
  if (int rc = c->vol.sst_partials.ensure(c, SST_MAX_PARTIALS)) return rc;
  const SegDev& s = c->vol.seg;
  const uint32_t* E = c->vol.dv.extent;
  const uint64_t* A = s.seg;
  const uint64_t* B = c->vol.slots[cp->slot].p;
  const size_t pairs = (size_t)s.nb * 4u;
  const uint32_t blocks = (uint32_t)std::min<size_t>((pairs + 255u) / 256u, SST_MAX_PARTIALS);
  SstCount* counts = c->vol.sst_partials;
  hipLaunchKernelGGL(sst_count, dim3(blocks), dim3(256), 0, c->stream, A, B, pairs, counts);
  hipLaunchKernelGGL(sst_count_final, dim3(1), dim3(256), 0, c->stream, counts, blocks);
  VX_HIP(c, hipGetLastError());
  DstPartial* tops = c->vol.dist_partials;   // with hausdorff: A over D2_B at [0], B over D2_A at [DST_MAX_PARTIALS / 2]
  if (cp->hausdorff) {
    // the field buffer is overwritten: whatever vx_segment_distance left there is gone
    c->vol.dist_valid = false;
    c->dst_launches = 0;
    // (event 4 is recorded twice, behind the first reduction and again ahead of the second x pass, as a two-round margin does)
    if (int rc = run_distance(c, B, 0ull, cp->spacing, DST_INF, 0)) return rc;
    if (int rc = launch_max_over(c, A, tops)) return rc;
    if (int rc = c->dst_timer.mark(c, 4)) return rc;
    if (int rc = run_distance(c, A, 0ull, cp->spacing, DST_INF, 4)) return rc;
    if (int rc = launch_max_over(c, B, tops + DST_MAX_PARTIALS / 2u)) return rc;
    if (int rc = mark_rest(c, 8, 9)) return rc;
  }
  SstCount n{};
  DstPartial top[2] = {{0ull, DST_NONE, 0.0f, 0u}, {0ull, DST_NONE, 0.0f, 0u}};
  VX_HIP(c, hipMemcpyAsync(&n, counts, sizeof n, hipMemcpyDeviceToHost, c->stream));
  if (cp->hausdorff) {
    VX_HIP(c, hipMemcpyAsync(&top[0], tops, sizeof top[0], hipMemcpyDeviceToHost, c->stream));
    VX_HIP(c, hipMemcpyAsync(&top[1], tops + DST_MAX_PARTIALS / 2u, sizeof top[1], hipMemcpyDeviceToHost, c->stream));
  }
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (cp->hausdorff)
    if (int rc = read_distance_times(c, 2)) return rc;
  VxCompareResult r{};
  r.count_a = n.a;
  r.count_b = n.b;
  r.count_and = n.ab;
  float* d2[2] = {&r.d2_ab, &r.d2_ba};
  uint32_t* arg[2] = {r.argmax_ab, r.argmax_ba};
  for (int k = 0; k < 2; ++k) {
    if (top[k].idx == DST_NONE) continue;   // its own set is empty (or hausdorff = 0): 0 and (0, 0, 0)
    *d2[k] = top[k].d2;
    arg[k][0] = (uint32_t)(top[k].idx % E[0]);
    arg[k][1] = (uint32_t)((top[k].idx / E[0]) % E[1]);
    arg[k][2] = (uint32_t)(top[k].idx / ((uint64_t)E[0] * E[1]));
  }
  if (out) *out = r;
  return VX_OK;
}

int vx_segments_labelmap(VxContext* c, const uint32_t* slots, uint32_t n, uint8_t* labels, uint64_t nvoxels, uint64_t* overlaps) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_segments_labelmap(c->members[0], slots, n, labels, nvoxels, overlaps));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_segments_labelmap", slots, "slots")) return rc;
  if (!labels) VX_FAIL(c, VX_ERR_INVALID, "vx_segments_labelmap: labels is NULL");
  if (n < 1u || n > VX_SEGMENT_SLOTS)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segments_labelmap: n = %u outside 1 .. %u (an empty or over-long list)", n, VX_SEGMENT_SLOTS);
  SstSlots list{};
  uint32_t listed = 0;
  for (uint32_t k = 0; k < n; ++k) {
    if (int rc = check_slot(c, "vx_segments_labelmap", slots[k], true)) return rc;
    if (listed & (1u << slots[k])) VX_FAIL(c, VX_ERR_INVALID, "vx_segments_labelmap: slot %u is listed twice (duplicate)", slots[k]);
    listed |= 1u << slots[k];
    list.w[k] = c->vol.slots[slots[k]].p;
  }
  list.n = n;
  const uint32_t* E = c->vol.dv.extent;
  const uint32_t* bc = c->vol.dv.bc;
  const size_t want = (size_t)E[0] * E[1] * E[2];
  if (nvoxels != want)
    VX_FAIL(c, VX_ERR_INVALID, "vx_segments_labelmap: nvoxels = %llu, the volume has %u x %u x %u = %zu voxels",
            (unsigned long long)nvoxels, E[0], E[1], E[2], want);
  if (int rc = c->vol.sst_labels.ensure(c, want)) return rc;   // (every earlier call has completed: each one synchronises)
  if (int rc = c->vol.sst_overlaps.ensure(c, 1)) return rc;
  unsigned long long* multi = c->vol.sst_overlaps;
  VX_HIP(c, hipMemsetAsync(multi, 0, sizeof *multi, c->stream));
  const uint32_t blocks = (uint32_t)std::min<size_t>((want / 8u + 255u) / 256u, 16384u);
  hipLaunchKernelGGL(sst_labelmap, dim3(blocks), dim3(256), 0, c->stream, list, bc[0], bc[1], bc[2], (uint8_t*)c->vol.sst_labels, multi);
  VX_HIP(c, hipGetLastError());
  unsigned long long over = 0;
  VX_HIP(c, hipMemcpyAsync(labels, c->vol.sst_labels, want, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipMemcpyAsync(&over, multi, sizeof over, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (overlaps) *overlaps = over;
  return VX_OK;
}

// ---- histograms ------------------------------------------------------------------------------------------------------------------
int vx_histogram(VxContext* c, const VxHistogramParams* hp, uint64_t* counts, uint32_t ncounts, VxHistogramResult* out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_histogram(c->members[0], hp, counts, ncounts, out));
  VX_DEV(c);
  VoxelBox box;
  if (int rc = check_ready(c, "vx_histogram", hp, "params")) return rc;
  if (hp->source < VX_HIST_VOLUME || hp->source > VX_HIST_SLOT)
    VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: source = %d is not a VxHistSource (0 .. 2)", hp->source);
  if (hp->source == VX_HIST_SEGMENT)
    if (int rc = check_current(c, "vx_histogram")) return rc;
  if (hp->source == VX_HIST_SLOT)
    if (int rc = check_slot(c, "vx_histogram", hp->slot, true)) return rc;
  if (int rc = check_box(c, "vx_histogram", hp->box_lo, hp->box_hi, &box)) return rc;
  HstParams h{};
  if (hp->rule == VX_HIST_LINEAR) {
    if (hp->bins < 1u || hp->bins > VX_HIST_MAX_BINS)
      VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: bins = %u outside 1 .. %u", hp->bins, VX_HIST_MAX_BINS);
    if (!std::isfinite(hp->lo)) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: lo is not finite");
    if (!std::isfinite(hp->hi)) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: hi is not finite");
    if (!(hp->lo < hp->hi)) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: lo = %g >= hi = %g", (double)hp->lo, (double)hp->hi);
    // (this unit is built without contraction: one rounded difference, one rounded quotient)
    const float width = hp->hi - hp->lo;
    h.inv = (float)hp->bins / width;
    if (!std::isfinite(h.inv))
      VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: hi - lo = %g is too narrow for bins = %u (bins / (hi - lo) is not finite)", (double)width,
              hp->bins);
    h.bins = hp->bins;
    h.lo = hp->lo;
    h.hi = hp->hi;
  } else if (hp->rule == VX_HIST_KEY) {
    const uint32_t p = hp->prefix_bits, b = hp->key_bits;
    if (b < 1u || b > VX_HIST_MAX_KEY_BITS) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: key_bits = %u outside 1 .. %u", b, VX_HIST_MAX_KEY_BITS);
    if (p > 31u) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: prefix_bits = %u outside 0 .. 31", p);
    if (p + b > 32u) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: prefix_bits + key_bits = %u + %u is more than the 32 bits of a key", p, b);
    if ((uint64_t)hp->prefix >= (1ull << p))
      VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: prefix = %u does not fit prefix_bits = %u", hp->prefix, p);
    h.bins = 1u << b;
    h.prefix = hp->prefix;
    h.top_shift = 32u - p;
    h.bin_shift = 32u - p - b;
    h.bin_mask = h.bins - 1u;
  } else {
    VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: rule = %d is not a VxHistRule (0 .. 1)", hp->rule);
  }
  h.rule = hp->rule;
  if (hp->moments != 0 && hp->moments != 1) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: moments = %d is not 0 or 1", hp->moments);
  if (!counts) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: counts is NULL");
  if (ncounts != h.bins) VX_FAIL(c, VX_ERR_INVALID, "vx_histogram: ncounts = %u, the call has %u bins", ncounts, h.bins);
  const bool moments = hp->moments != 0;
  // the brick grid from the volume itself: VX_HIST_VOLUME needs no segment, so SegDev may not be there
  const uint32_t* bc = c->vol.dv.bc;
  h.nb = bc[0] * bc[1] * bc[2];
  for (int a = 0; a < 3; ++a) {
    h.bc[a] = bc[a];
    h.box_lo[a] = box.lo[a];
    h.box_hi[a] = box.hi[a];
  }
  h.mask = hp->source == VX_HIST_SEGMENT ? c->vol.seg.seg : hp->source == VX_HIST_SLOT ? c->vol.slots[hp->slot].p : nullptr;
  // (every earlier call has completed: each one synchronises)
  if (int rc = c->vol.hst_bins.ensure(c, VX_HIST_MAX_BINS + 2u)) return rc;
  if (moments)
    if (int rc = c->vol.hst_partials.ensure(c, (size_t)h.nb + 1u)) return rc;
  h.out = c->vol.hst_bins;
  h.partial = moments ? c->vol.hst_partials.p : nullptr;
  const size_t slots = (size_t)h.bins + 2u;
  VX_HIP(c, hipMemsetAsync(h.out, 0, slots * sizeof(unsigned long long), c->stream));
  if (int rc = c->hst_timer.mark(c, 0)) return rc;
  launch_hst_bins(c, h, moments, std::min<uint32_t>((h.nb + 3u) / 4u, HST_MAX_BLOCKS));
  VX_HIP(c, hipGetLastError());
  if (int rc = c->hst_timer.mark(c, 1)) return rc;
  if (moments) {
    hipLaunchKernelGGL(hst_moments, dim3(1), dim3(1024), 0, c->stream, (const HstPartial*)h.partial, h.nb, h.partial + h.nb);
    VX_HIP(c, hipGetLastError());
  }
  if (int rc = c->hst_timer.mark(c, 2)) return rc;
  std::vector<unsigned long long> got(slots);
  HstPartial total{};
  VX_HIP(c, hipMemcpyAsync(got.data(), h.out, slots * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  if (moments) VX_HIP(c, hipMemcpyAsync(&total, h.partial + h.nb, sizeof total, hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->hst_timer.read(c)) return rc;
  if (!moments) c->hst_timer.ms[1] = 0.0;   // (two events back to back still measure a few microseconds)
  c->hst_launches = moments ? 2u : 1u;
  VxHistogramResult r{};
  r.below = got[h.bins];
  r.above = got[h.bins + 1u];
  r.count = r.below + r.above;
  for (uint32_t k = 0; k < h.bins; ++k) {
    counts[k] = got[k];
    r.count += got[k];
  }
  if (moments && r.count) {
    r.d_sum = total.sum;
    r.d_sum2 = total.sum2;
    r.d_min = total.mn;
    r.d_max = total.mx;
  }
  if (out) *out = r;
  return VX_OK;
}

int vx_histogram_stats(VxContext* c, uint32_t* launches, double* kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_histogram_stats(c->members[0], launches, kernel_ms));
  if (launches) *launches = c->hst_launches;
  if (kernel_ms) std::copy_n(c->hst_timer.ms, 2, kernel_ms);
  return VX_OK;
}

}  // extern "C"
