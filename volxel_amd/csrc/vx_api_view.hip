// vx_api_view.hip -- the view unit of the host layer (units: DESIGN.md section 4.1): multiplanar slices and thick slabs
// (vx_slice) and first-hit isosurfaces (vx_isosurface), with their statistics.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <vector>

#include "vx_slice.hpp"
#include "vx_iso.hpp"
#include "vx_context.hpp"

using namespace vx;

namespace {

// ---- slices (vx_slice): the kernel a slice runs, chosen apart from plan_launch (a slice is no render launch) ---------------
// launches slice_reduce<sp.reduce, the layout of slice_layout> for sp on the context's stream
static void launch_slice(VxContext* c, const VxSliceParams& sp) {
  const dim3 grid((sp.size[0] + 15u) / 16u, (sp.size[1] + 15u) / 16u);
  const VxParams& p = c->params;
  with_layout(slice_layout(c), [&](auto lay) {
    constexpr int LAY = decltype(lay)::value;
    auto go = [&](auto red) {
      hipLaunchKernelGGL((slice_reduce<decltype(red)::value, LAY>), grid, dim3(256), 0, c->stream, sp, c->vol.dv, p.volume_density_scale,
                         p.volume_inv_maj, c->tf, c->tf_len, p.sample_range[0], p.sample_range[1], c->slice_values, c->slice_rgba);
    };
    if (sp.reduce == VX_SLICE_MAX) go(std::integral_constant<int, VX_SLICE_MAX>{});
    else if (sp.reduce == VX_SLICE_MIN) go(std::integral_constant<int, VX_SLICE_MIN>{});
    else go(std::integral_constant<int, VX_SLICE_MEAN>{});
  });
}

// ---- isosurfaces (vx_isosurface): the upper density bounds of range skipping and the launch --------------------------------
// The projections' bound table (compute_projection_bounds, its widening argument included), upper bounds only, kept in a buffer
// of its own: building it never marks, frees or replaces the table MIP / MinIP launches read (proj_table / proj_dev).
static int rebuild_iso_bounds(VxContext* c) {
  const VxParams& p = c->params;
  c->vol.iso_table.stale = true;   // until this build is complete
  std::vector<float> lohi;
  int level = 1;
  uint32_t md[3];
  compute_projection_bounds(p, c->range_host.data(), c->vol.dv.bc, c->vol.dv.extent, lohi, level, md);
  const size_t n = lohi.size() / 2;
  std::vector<float> hi(n);
  for (size_t i = 0; i < n; ++i) hi[i] = lohi[2 * i + 1];
  if (int rc = c->iso_bound_dev.alloc(c, n)) return rc;
  VX_HIP(c, hipMemcpyAsync(c->iso_bound_dev, hi.data(), n * sizeof(float), hipMemcpyHostToDevice, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  IsoBound& b = c->iso_bound;
  b.hi = c->iso_bound_dev;
  b.sh = 3u + (uint32_t)level;
  b.md0 = md[0];
  b.md1 = md[1];
  for (int a = 0; a < 3; ++a) b.cmax[a] = c->vol.dv.extent[a] + 7u;
  c->vol.iso_table.built(p);
  return VX_OK;
}
// launches iso_first_hit<the layout of slice_layout, ip.skip> over the window (x0, y0, ww, wh) on the context's stream
// (the segment view: iso_first_hit_seg<the layout of slice_layout>, never skipping)
static void launch_iso(VxContext* c, const VxIsoParams& ip, uint32_t ww, uint32_t wh) {
  const dim3 grid((ww + 15u) / 16u, (wh + 15u) / 16u);
  with_layout(slice_layout(c), [&](auto lay) {
    constexpr int LAY = decltype(lay)::value;
    if (c->vol.seg_view != VX_SEGVIEW_OFF)
      hipLaunchKernelGGL((iso_first_hit_seg<LAY>), grid, dim3(256), 0, c->stream, c->params, c->vol.dv, ip, c->iso_rgba, c->iso_hit,
                         c->iso_count_dev, reinterpret_cast<const uint32_t*>(c->vol.seg.seg), c->vol.seg_view == VX_SEGVIEW_HIDE ? ~0u : 0u);
    else if (ip.skip)
      hipLaunchKernelGGL((iso_first_hit<LAY, true>), grid, dim3(256), 0, c->stream, c->params, c->vol.dv, ip, c->iso_bound, c->iso_rgba,
                         c->iso_hit, c->iso_count_dev);
    else
      hipLaunchKernelGGL((iso_first_hit<LAY, false>), grid, dim3(256), 0, c->stream, c->params, c->vol.dv, ip, IsoBound{}, c->iso_rgba,
                         c->iso_hit, c->iso_count_dev);
  });
}

}  // namespace

extern "C" {

int vx_slice(VxContext* c, const VxSliceParams* sp, float* values_out, uint8_t* rgba8_out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_slice(c->members[0], sp, values_out, rgba8_out));
  VX_DEV(c);
  if (int rc = check_ready(c, "vx_slice", sp, "sp")) return rc;
  if (int rc = check_slice_size(c, "vx_slice", sp)) return rc;
  if (sp->reduce < VX_SLICE_MEAN || sp->reduce > VX_SLICE_MIN) VX_FAIL(c, VX_ERR_INVALID, "vx_slice: unknown reduce %d", sp->reduce);
  if (sp->display < VX_SLICE_NONE || sp->display > VX_SLICE_TF)
    VX_FAIL(c, VX_ERR_INVALID, "vx_slice: unknown display %d", sp->display);
  if (int rc = check_slice_frame(c, "vx_slice", sp)) return rc;
  if (sp->display == VX_SLICE_GREY &&
      !(std::isfinite(sp->window[0]) && std::isfinite(sp->window[1]) && sp->window[1] > sp->window[0]))
    VX_FAIL(c, VX_ERR_INVALID, "vx_slice: window [%g, %g] with VX_SLICE_GREY: needs finite window[0] < window[1]",
            (double)sp->window[0], (double)sp->window[1]);
  if (sp->display == VX_SLICE_TF && !c->tf)
    VX_FAIL(c, VX_ERR_INVALID, "vx_slice: display VX_SLICE_TF without a transfer function (vx_upload_transfer first)");
  if (rgba8_out && sp->display == VX_SLICE_NONE)
    VX_FAIL(c, VX_ERR_INVALID, "vx_slice: rgba8_out with display VX_SLICE_NONE (no display output)");
  const size_t px = (size_t)sp->size[0] * sp->size[1];
  // (every earlier slice has completed: vx_slice synchronises)
  if (int rc = c->slice_values.ensure(c, px)) return rc;
  if (int rc = c->slice_rgba.ensure(c, px)) return rc;
  if (int rc = c->slice_timer.mark(c, 0)) return rc;
  launch_slice(c, *sp);
  VX_HIP(c, hipGetLastError());
  if (int rc = c->slice_timer.mark(c, 1)) return rc;
  if (values_out)
    VX_HIP(c, hipMemcpyAsync(values_out, c->slice_values, px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
  if (rgba8_out) VX_HIP(c, hipMemcpyAsync(rgba8_out, c->slice_rgba, px * sizeof(uchar4), hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->slice_timer.read(c)) return rc;
  c->slice_samples = (uint64_t)px * sp->slab_samples;
  return VX_OK;
}

int vx_slice_stats(VxContext* c, uint64_t* samples, double* last_kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_slice_stats(c->members[0], samples, last_kernel_ms));
  if (samples) *samples = c->slice_samples;
  if (last_kernel_ms) *last_kernel_ms = c->slice_timer.ms[0];
  return VX_OK;
}

int vx_isosurface(VxContext* c, const VxIsoParams* ip, float* rgba_out, float* hit_out) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_isosurface(c->members[0], ip, rgba_out, hit_out));
  VX_DEV(c);
  if (!c->vol.has_volume) VX_FAIL(c, VX_ERR_NO_VOLUME, "vx_isosurface: no volume uploaded");
  if (!c->has_params) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: vx_set_params first (the camera, clip box and march come from it)");
  if (!ip) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: ip is NULL");
  // the march of any render mode's params: the checks vx_set_params makes for the marching modes
  if (!(c->params.dvr_step_voxels > 0.0f)) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: params.dvr_step_voxels must be > 0");
  if (c->params.dvr_max_steps < 0 || c->params.dvr_max_steps > (1 << 24))
    VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: params.dvr_max_steps %d outside [0, 2^24]", c->params.dvr_max_steps);
  const struct { const char* name; float v; } terms[8] = {{"iso", ip->iso}, {"color[0]", ip->color[0]}, {"color[1]", ip->color[1]},
                                                          {"color[2]", ip->color[2]}, {"ka", ip->ka}, {"kd", ip->kd},
                                                          {"ks", ip->ks}, {"shininess", ip->shininess}};
  for (const auto& e : terms)
    if (!std::isfinite(e.v)) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: %s is not finite", e.name);
  if (ip->shininess < 0.0f) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: shininess = %g < 0", (double)ip->shininess);
  if (ip->refine > 16u) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: refine = %u outside 0 .. 16", ip->refine);
  if (ip->skip != 0 && ip->skip != 1) VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: skip = %d is not 0 or 1", ip->skip);
  const uint32_t W = (uint32_t)c->params.res[0], H = (uint32_t)c->params.res[1];
  VxIsoParams q = *ip;
  if (!q.window[0] && !q.window[1] && !q.window[2] && !q.window[3]) {
    q.window[2] = W;
    q.window[3] = H;
  }
  if (!(q.window[0] < q.window[2] && q.window[1] < q.window[3] && q.window[2] <= W && q.window[3] <= H))
    VX_FAIL(c, VX_ERR_INVALID, "vx_isosurface: window (%u, %u, %u, %u) is empty or outside the render size %u x %u", q.window[0],
            q.window[1], q.window[2], q.window[3], W, H);
  const uint32_t ww = q.window[2] - q.window[0], wh = q.window[3] - q.window[1];
  const size_t px = (size_t)ww * wh;
  // (every earlier call has completed: vx_isosurface synchronises)
  if (int rc = c->iso_rgba.ensure(c, px)) return rc;
  if (int rc = c->iso_hit.ensure(c, px)) return rc;
  if (int rc = check_segment_view(c, "vx_isosurface", true)) return rc;
  if (c->vol.seg_view != VX_SEGVIEW_OFF) q.skip = 0;   // masked: no range skipping
  if (q.skip && !c->vol.iso_table.current(c->params)) {
    const int rc = rebuild_iso_bounds(c);
    if (rc) return rc;
  }
  if (int rc = c->iso_count_dev.ensure(c, ISO_NCOUNTS)) return rc;
  VX_HIP(c, hipMemsetAsync(c->iso_count_dev, 0, ISO_NCOUNTS * sizeof(unsigned long long), c->stream));
  if (int rc = c->iso_timer.mark(c, 0)) return rc;
  launch_iso(c, q, ww, wh);
  VX_HIP(c, hipGetLastError());
  if (int rc = c->iso_timer.mark(c, 1)) return rc;
  uint64_t counts[ISO_NCOUNTS];
  VX_HIP(c, hipMemcpyAsync(counts, c->iso_count_dev, sizeof counts, hipMemcpyDeviceToHost, c->stream));
  if (rgba_out) VX_HIP(c, hipMemcpyAsync(rgba_out, c->iso_rgba, px * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  if (hit_out) VX_HIP(c, hipMemcpyAsync(hit_out, c->iso_hit, px * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
  VX_HIP(c, hipStreamSynchronize(c->stream));
  if (int rc = c->iso_timer.read(c)) return rc;
  memcpy(c->iso_counts, counts, sizeof counts);
  return VX_OK;
}

int vx_iso_stats(VxContext* c, uint64_t* rays, uint64_t* hits, uint64_t* samples, uint64_t* refine_samples, uint64_t* skipped,
                 double* last_kernel_ms) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_iso_stats(c->members[0], rays, hits, samples, refine_samples, skipped, last_kernel_ms));
  if (rays) *rays = c->iso_counts[ISO_RAYS];
  if (hits) *hits = c->iso_counts[ISO_HITS];
  if (samples) *samples = c->iso_counts[ISO_SAMPLES];
  if (refine_samples) *refine_samples = c->iso_counts[ISO_REFINE];
  if (skipped) *skipped = c->iso_counts[ISO_SKIPPED];
  if (last_kernel_ms) *last_kernel_ms = c->iso_timer.ms[0];
  return VX_OK;
}

}  // extern "C"
