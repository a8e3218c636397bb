// vx_api_volume.hip -- the volume unit of the host layer (units: DESIGN.md section 4.1): getting a volume onto the device
// (vx_upload_volume, vx_upload_brick_grid, vx_upload_stats) and keeping its sampled layouts resident (vx_set_layout, and
// ensure_layout for the render unit, which decides what a launch samples).  The build_* layout kernels are instantiated here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <vector>

#include "../../include/volxel_brick.h"
#include "vx_layout.hpp"
#include "vx_context.hpp"

using namespace vx;

namespace {

// ---- the native layouts: one description each, used by every path that allocates or fills one ------------------------------
// A layout on the brick grid of `dv`: its z layers (brick layers; cellquad: layers of the apron-brick grid bc + 1), which are
// contiguous, the elements per layer and in all (brickf32: voxels; bricku8: dwords of four codes; cellquad: quads), and whether the
// kernels that sample it can index them.  The reference textures have no layers.
struct LayoutDesc { uint32_t layers; uint64_t per_layer, n; bool indexable; };
static LayoutDesc describe(const DevVolume& dv, int layout) {
  const uint64_t bricks_xy = (uint64_t)dv.bc[0] * dv.bc[1];
  LayoutDesc d{};
  if (layout == VX_LAYOUT_BRICKF32) d = {dv.bc[2], bricks_xy * 512u};
  if (layout == VX_LAYOUT_BRICKU8) d = {dv.bc[2], bricks_xy * 128u};
  if (layout == VX_LAYOUT_CELLQUAD) d = {dv.bc[2] + 1, (uint64_t)(dv.bc[0] + 1) * (dv.bc[1] + 1) * CQ_BRICK_QUADS};
  d.n = d.per_layer * d.layers;
  // brickf32: the staging loads index the layout in 16-byte units with 32 bits: 64 GiB, about 2500^3 voxels; bricku8: its dwords;
  // cellquad: the march indexes quads with 32 bits (and bricks with 24-bit multiplies): 64 GiB, about 1550^3 voxels
  d.indexable = layout == VX_LAYOUT_BRICKF32 ? !(d.n / 4u > 0xffffffffull)
              : layout == VX_LAYOUT_BRICKU8 ? !(d.n > 0xfffffff0ull) : !(d.n > 0xffffffffull);
  return d;
}

// Allocate one layout beside what is resident, zero what lies behind its last element, and point DevVolume at it; fill_layout
// writes the contents.  A volume beyond the layout's index range is refused here, with the layouts that take it.
static int alloc_one_layout(VxContext* c, int layout) {
  VxContext::Volume& vol = c->vol;
  DevVolume& dv = vol.dv;
  const LayoutDesc d = describe(dv, layout);
  if (layout == VX_LAYOUT_BRICKF32) {
    if (!d.indexable)
      VX_FAIL(c, VX_ERR_INVALID, "volume too large for the brickf32 layout (%llu voxels): select VX_LAYOUT_REFERENCE "
              "with vx_set_layout", (unsigned long long)d.n);
    // + one zero 16-byte chunk behind the last brick: the window staging of the LDS kernel reads it for rows and
    // chunks outside the volume (one select per load instead of a branch and a zero fill); it finds the chunk, and
    // bricku8's zero unit, at unit bricks * 128 (zero_chunk, vx_dvr_lds_march.inc): right behind the d.n elements
    if (int rc = vol.bf_alloc.alloc(c, d.n * sizeof(float) + 16)) return rc;
    VX_HIP(c, hipMemsetAsync((char*)vol.bf_alloc.p + d.n * sizeof(float), 0, 16, c->stream));
    dv.bf = (const float*)vol.bf_alloc.p;
    dv.bf_zero = d.n <= 0xfffffff0ull ? (uint32_t)d.n : 0u;
  } else if (layout == VX_LAYOUT_BRICKU8) {
    const uint64_t n_bricks = d.n / 128u;
    if (!d.indexable)
      VX_FAIL(c, VX_ERR_INVALID, "volume too large for the bricku8 layout (%llu bricks): select VX_LAYOUT_REFERENCE "
              "with vx_set_layout", (unsigned long long)n_bricks);
    // + one zero unit behind the last brick and its {0, 0} range: rows and chunks outside the volume decode to +0
    if (int rc = vol.bu_alloc.alloc(c, (d.n + 4u) * sizeof(uint32_t))) return rc;
    if (int rc = vol.bur_alloc.alloc(c, (n_bricks + 1u) * sizeof(float2))) return rc;
    VX_HIP(c, hipMemsetAsync((char*)vol.bu_alloc.p + d.n * sizeof(uint32_t), 0, 4u * sizeof(uint32_t), c->stream));
    VX_HIP(c, hipMemsetAsync((char*)vol.bur_alloc.p + n_bricks * sizeof(float2), 0, sizeof(float2), c->stream));
    dv.bu = (const uint32_t*)vol.bu_alloc.p;
    dv.bu_range = (const float2*)vol.bur_alloc.p;
  } else if (layout == VX_LAYOUT_CELLQUAD) {
    for (int i = 0; i < 3; ++i) dv.cq_bc[i] = dv.bc[i] + 1;
    if (!d.indexable)
      VX_FAIL(c, VX_ERR_INVALID,
              "volume too large for the cellquad layout (%llu quads > 2^32): select VX_LAYOUT_BRICKF32 or "
              "VX_LAYOUT_REFERENCE with vx_set_layout", (unsigned long long)d.n);
    if (int rc = vol.cq_alloc.alloc(c, d.n * sizeof(float4))) return rc;
    dv.cq = (const float4*)vol.cq_alloc.p;
  }
  return VX_OK;
}

// kernel(dv, out, at, at + n) over [first, end) on `st`, one thread per element, at most 2^31 threads per launch
template <class T, class I>
static void launch_range(void (*kernel)(DevVolume, T*, I, I), const DevVolume& dv, void* out, uint64_t first, uint64_t end,
                         hipStream_t st) {
  for (uint64_t at = first; at < end;) {
    const uint64_t n = std::min<uint64_t>(end - at, 1ull << 31);
    hipLaunchKernelGGL(kernel, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, st, dv, (T*)out, (I)at, (I)(at + n));
    at += n;
  }
}

// fill z layers [z0, z1) of an allocated layout on `st`
static int fill_layout(VxContext* c, int layout, uint32_t z0, uint32_t z1, hipStream_t st) {
  if (z1 <= z0) return VX_OK;
  const VxContext::Volume& vol = c->vol;
  const uint64_t per = describe(vol.dv, layout).per_layer, first = per * z0, end = per * z1;
  if (layout == VX_LAYOUT_BRICKF32) {
    launch_range(build_brickf32, vol.dv, vol.bf_alloc.p, first, end, st);
  } else if (layout == VX_LAYOUT_BRICKU8) {
    launch_range(build_bricku8, vol.dv, vol.bu_alloc.p, first, end, st);
    launch_range(build_bricku8_range, vol.dv, vol.bur_alloc.p, first / 128u, end / 128u, st);   // bricks: < 2^30
  } else if (layout == VX_LAYOUT_CELLQUAD) {
    launch_range(build_cellquad, vol.dv, vol.cq_alloc.p, first, end, st);
  }
  VX_HIP(c, hipGetLastError());
  return VX_OK;
}

// allocate one layout and fill all of it on the context's stream
static int build_one_layout(VxContext* c, int layout) {
  if (int rc = alloc_one_layout(c, layout)) return rc;
  return fill_layout(c, layout, 0, describe(c->vol.dv, layout).layers, c->stream);
}

// Drop every layout and note what the volume's size allows under VX_LAYOUT_AUTO; primary_layout then names the layout the
// upload builds behind its copies and vx_set_layout builds whole.
static void reset_layouts(VxContext* c) {
  VxContext::Volume& vol = c->vol;
  for (DevBuf<void>* b : {&vol.cq_alloc, &vol.bf_alloc, &vol.bu_alloc, &vol.bur_alloc}) b->reset();
  vol.dv.cq = nullptr, vol.dv.bf = nullptr, vol.dv.bf_zero = 0;
  vol.dv.bu = nullptr, vol.dv.bu_range = nullptr;
  c->auto_no_bf = c->layout == VX_LAYOUT_AUTO && !describe(vol.dv, VX_LAYOUT_BRICKF32).indexable;
  c->auto_no_cq = c->layout == VX_LAYOUT_AUTO && !describe(vol.dv, VX_LAYOUT_CELLQUAD).indexable;
}

// Pin a caller-owned host range for the duration of an upload so that the copy engine reads it directly at
// PCIe rate ("pin/upload volumes to HBM", BASELINE north star).  Pageable memory would be staged through the
// runtime's bounce buffers at a fraction of that.  Failing to pin (already registered, locked-memory limit)
// is not an error: the copies then go the pageable way.
struct PinnedRange {
  void* p = nullptr;
  bool pinned = false;
  PinnedRange(const void* ptr, size_t bytes) {
    if (!ptr || bytes < (1u << 20)) return;
    p = const_cast<void*>(ptr);
    hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    pinned = (e == hipSuccess);
    if (!pinned) (void)hipGetLastError();   // clear the sticky error
  }
  ~PinnedRange() {
    if (pinned) (void)hipHostUnregister(p);
  }
};

}  // namespace

void vx::free_volume(VxContext* c) {
  for (void* p : c->vol_allocs) (void)hipFree(p);
  c->vol_allocs.clear();
  c->vol = VxContext::Volume{};
}

int vx::ensure_layout(VxContext* c, int layout) {
  const DevVolume& dv = c->vol.dv;
  if (layout == VX_LAYOUT_CELLQUAD ? dv.cq != nullptr : dv.bf != nullptr) return VX_OK;
  const LayoutDesc d = describe(dv, layout);
  if (!d.indexable) return VX_OK;   // brickf32 for Phong beside cellquad: the generic kernel serves it
  if (layout == VX_LAYOUT_CELLQUAD && c->layout == VX_LAYOUT_AUTO) {
    // AUTO builds this layout on demand, beside what is resident: only when it leaves half of the free device memory to
    // the rest of the process (19.8 GB for 1024^3 on a 288 GB MI355X: always; a volume near the layout's 64 GiB index limit
    // on a device that other contexts share: not necessarily).  Otherwise `default` / `no_dda` take the resident bricks.
    // VX_AUTO_CELLQUAD_MAX_BYTES (Switches) overrides the budget -- 0 keeps AUTO off this layout.
    size_t free_b = 0, total_b = 0;
    VX_HIP(c, hipMemGetInfo(&free_b, &total_b));
    const uint64_t budget = c->sw.cellquad_max_bytes.value_or((uint64_t)free_b / 2u);
    if (d.n * sizeof(float4) > budget) {
      c->auto_no_cq = true;
      return VX_OK;
    }
  }
  return build_one_layout(c, layout);
}

extern "C" {

int vx_upload_volume(VxContext* c, const uint32_t* indirection, const uint32_t ind_size[3],
                     const uint16_t* range, const uint32_t range_size[3], const uint8_t* atlas,
                     const uint32_t atlas_size[3], int n_mips, const uint16_t* const* mip_data,
                     const uint32_t (*mip_size)[3], const uint32_t index_extent[3]) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c))
    return fan_out(c, [&](VxContext* m, size_t) {
      return vx_upload_volume(m, indirection, ind_size, range, range_size, atlas, atlas_size, n_mips, mip_data, mip_size,
                              index_extent);
    });
  VX_DEV(c);
  if (!indirection || !range || !ind_size || !range_size || !atlas_size || !index_extent)
    VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: null argument");
  if (n_mips != 3 || !mip_data || !mip_size)
    VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: expected 3 range mipmaps (brick.rs:13)");
  for (int i = 0; i < 3; ++i) {
    if (ind_size[i] != range_size[i] || ind_size[i] == 0 || ind_size[i] >= 1024u)
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: bad brick grid dimensions");
    if (index_extent[i] != ind_size[i] * 8u)
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: index_extent must be brick_count*8 (brick.rs:236-238)");
    if (i < 2 && atlas_size[i] != ind_size[i] * 8u)
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: atlas x/y dims must be brick_count*8 (brick.rs:85)");
  }
  if (atlas_size[2] % 8u != 0 || atlas_size[2] > ind_size[2] * 8u)
    VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: bad atlas depth");
  size_t atlas_bytes = (size_t)atlas_size[0] * atlas_size[1] * atlas_size[2];
  if (atlas_bytes && !atlas) VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: null atlas");
  for (int k = 0; k < 3; ++k) {
    if (!mip_data[k] && (size_t)mip_size[k][0] * mip_size[k][1] * mip_size[k][2])
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: null mip %d", k);
    if (mip_size[k][0] != (ind_size[0] >> (k + 1)) || mip_size[k][1] != (ind_size[1] >> (k + 1)) ||
        mip_size[k][2] != (ind_size[2] >> (k + 1)))
      VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: mip %d has wrong dimensions (brick.rs:156)", k);
  }
  const auto t_begin = std::chrono::steady_clock::now();
  VX_HIP(c, hipStreamSynchronize(c->stream));
  free_volume(c);
  const size_t nb = (size_t)ind_size[0] * ind_size[1] * ind_size[2];
  const size_t per_layer = (size_t)ind_size[0] * ind_size[1];
  // every pointer must address an allocated atlas brick; while scanning, note how many 8-slice atlas layers
  // the bricks of each brick z layer reach into (the builder allocates slots in scan order, brick.rs:127-129,
  // so this grows with z and the layout of early layers can be built while the rest of the atlas still copies)
  std::vector<uint32_t> reach(ind_size[2], 0u);
  {
    const uint32_t max_slot = atlas_size[2] / 8u;
    for (size_t i = 0; i < nb; ++i) {
      uint32_t p = indirection[i];
      uint32_t az = (p >> 20) & 1023u;
      if ((p & 1023u) >= ind_size[0] || ((p >> 10) & 1023u) >= ind_size[1] || (az >= max_slot && p != 0))
        VX_FAIL(c, VX_ERR_INVALID, "vx_upload_volume: indirection pointer outside the atlas");
      uint32_t& r = reach[i / per_layer];
      if (max_slot && az + 1u > r) r = az + 1u;   // constant bricks alias slot 0 (quirk Q6): also fine
    }
    for (uint32_t z = 1; z < ind_size[2]; ++z) reach[z] = reach[z] > reach[z - 1] ? reach[z] : reach[z - 1];
  }
  auto alloc = [&](size_t bytes, void** dst) -> int {
    *dst = nullptr;
    if (bytes == 0) return VX_OK;
    VX_HIP(c, hipMalloc(dst, bytes));
    c->vol_allocs.push_back(*dst);
    return VX_OK;
  };
  void *d_ind = nullptr, *d_range = nullptr, *d_atlas = nullptr, *d_mip[3] = {nullptr, nullptr, nullptr};
  int rc;
  // the atlas allocation is never empty: a tap that points outside the pruned atlas reads byte 0 and selects 0
  // (lookup_density_brick is straight-line code)
  if ((rc = alloc(nb * 4, &d_ind)) || (rc = alloc(nb * 4, &d_range)) || (rc = alloc(atlas_bytes ? atlas_bytes : 16, &d_atlas))) { free_volume(c); return rc; }
  if (!atlas_bytes) VX_HIP(c, hipMemsetAsync(d_atlas, 0, 16, c->stream));
  size_t mip_n[3];
  for (int k = 0; k < 3; ++k) {
    mip_n[k] = (size_t)mip_size[k][0] * mip_size[k][1] * mip_size[k][2];
    if ((rc = alloc(mip_n[k] * 4, &d_mip[k]))) { free_volume(c); return rc; }
    c->vol.dv.mips[k] = (const uint32_t*)d_mip[k];
    for (int i = 0; i < 3; ++i) c->vol.dv.mip_size[k][i] = mip_size[k][i];
  }
  c->vol.dv.indirection = (const uint32_t*)d_ind;
  c->vol.dv.range = (const uint32_t*)d_range;   // u16 stream [max,min] == LE u32 (min<<16)|max
  c->vol.dv.atlas = (const uint8_t*)d_atlas;
  for (int i = 0; i < 3; ++i) {
    c->vol.dv.bc[i] = ind_size[i];
    c->vol.dv.atlas_size[i] = atlas_size[i];
    c->vol.dv.extent[i] = index_extent[i];
  }
  c->range_host.assign((const uint32_t*)range, (const uint32_t*)range + nb);
  c->vol.skip_table.stale = c->vol.proj_table.stale = c->vol.iso_table.stale = true;
  c->order_builds_left = 2;
  reset_layouts(c);
  const int lay = primary_layout(c);
  if ((rc = alloc_one_layout(c, lay))) { free_volume(c); return rc; }
  const uint32_t n_layers = describe(c->vol.dv, lay).layers;
  if (!c->aux_stream) VX_HIP(c, hipStreamCreateWithFlags(&c->aux_stream, hipStreamNonBlocking));

  // ---- copies: metadata first, then the atlas in chunks of whole 8-slice layers from pinned memory;
  //      the layout layers whose bricks are complete are built on the aux stream behind each chunk
  // Every failure from here on goes through ONE exit (below): both streams are synchronised before the pinned
  // ranges are unregistered and the partial volume is freed -- an early return would unpin pages an earlier
  // asynchronous copy may still be reading.
  PinnedRange pin_atlas(atlas, atlas_bytes), pin_ind(indirection, nb * 4), pin_range(range, nb * 4);
  hipError_t le = hipMemcpyAsync(d_ind, indirection, nb * 4, hipMemcpyHostToDevice, c->stream);
  if (le == hipSuccess) le = hipMemcpyAsync(d_range, range, nb * 4, hipMemcpyHostToDevice, c->stream);
  for (int k = 0; k < 3 && le == hipSuccess; ++k)
    if (mip_n[k]) le = hipMemcpyAsync(d_mip[k], mip_data[k], mip_n[k] * 4, hipMemcpyHostToDevice, c->stream);
  const uint32_t atlas_layers = atlas_size[2] / 8u;
  const size_t layer_bytes = (size_t)atlas_size[0] * atlas_size[1] * 8u;
  const uint32_t chunk_layers = layer_bytes ? (uint32_t)std::max<size_t>(1, (16u << 20) / layer_bytes) : 1u;
  std::vector<hipEvent_t> evs;
  uint32_t built = 0;     // layout layers launched so far
  auto buildable = [&](uint32_t copied) {   // layout layers whose source bricks lie in the copied atlas prefix
    uint32_t z = built;
    while (z < n_layers) {
      // cellquad apron layer z reads brick layers z-1 and z; brickf32 layer z reads brick layer z
      uint32_t top = z < ind_size[2] ? z : ind_size[2] - 1u;
      if (reach[top] > copied) break;
      ++z;
    }
    return z;
  };
  // layout layers [built, z1) on the aux stream, behind what the context's stream has copied so far
  auto build_behind_copies = [&](uint32_t z1) -> hipError_t {
    hipEvent_t e;
    hipError_t he = hipEventCreateWithFlags(&e, hipEventDisableTiming);
    if (he != hipSuccess) return he;
    evs.push_back(e);
    if ((he = hipEventRecord(e, c->stream)) != hipSuccess) return he;
    if ((he = hipStreamWaitEvent(c->aux_stream, e, 0)) != hipSuccess) return he;
    if ((rc = fill_layout(c, lay, built, z1, c->aux_stream))) return hipErrorUnknown;
    built = z1;
    return hipSuccess;
  };
  for (uint32_t l0 = 0; l0 < atlas_layers && le == hipSuccess; l0 += chunk_layers) {
    uint32_t l1 = l0 + chunk_layers < atlas_layers ? l0 + chunk_layers : atlas_layers;
    le = hipMemcpyAsync((char*)d_atlas + l0 * layer_bytes, atlas + l0 * layer_bytes, (l1 - l0) * layer_bytes,
                        hipMemcpyHostToDevice, c->stream);
    if (le != hipSuccess) break;
    uint32_t z1 = buildable(l1);
    if (z1 > built && l1 < atlas_layers) le = build_behind_copies(z1);   // the last chunk's layers go with the final build below
  }
  if (le == hipSuccess && built < n_layers) le = build_behind_copies(n_layers);
  hipError_t s1 = hipStreamSynchronize(c->stream);    // host buffers may be dropped on return
  hipError_t s2 = hipStreamSynchronize(c->aux_stream);
  for (hipEvent_t e : evs) (void)hipEventDestroy(e);
  if (le != hipSuccess || s1 != hipSuccess || s2 != hipSuccess) {
    hipError_t bad = le != hipSuccess ? le : (s1 != hipSuccess ? s1 : s2);
    free_volume(c);
    VX_FAIL(c, VX_ERR_DEVICE, "vx_upload_volume: %s", hipGetErrorString(bad));
  }
  c->vol.has_volume = true;
  c->upload_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_begin).count();
  c->upload_host_bytes = (uint64_t)atlas_bytes + (uint64_t)nb * 8u + (uint64_t)(mip_n[0] + mip_n[1] + mip_n[2]) * 4u;
  c->upload_pinned = pin_atlas.pinned ? 1 : 0;
  return VX_OK;
}

int vx_upload_stats(VxContext* c, double* seconds, uint64_t* host_bytes, int* pinned) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return on_member0(c, vx_upload_stats(c->members[0], seconds, host_bytes, pinned));
  if (seconds) *seconds = c->upload_seconds;
  if (host_bytes) *host_bytes = c->upload_host_bytes;
  if (pinned) *pinned = c->upload_pinned;
  return VX_OK;
}

int vx_upload_brick_grid(VxContext* c, const VxBrickGrid* g) {
  if (!c) return VX_ERR_INVALID;
  if (!g) VX_FAIL(c, VX_ERR_INVALID, "vx_upload_brick_grid: null grid");
  uint32_t is[3], rs[3], as[3], ext[3], ms[3][3];
  vxb_indirection_size(g, is);
  vxb_range_size(g, rs);
  vxb_atlas_size(g, as);
  vxb_index_extent(g, ext);
  const uint32_t n = vxb_range_mipmaps(g);
  if (n != 3) VX_FAIL(c, VX_ERR_INVALID, "vx_upload_brick_grid: grid has %u range mips, expected 3", n);
  const uint16_t* mips[3];
  for (uint32_t i = 0; i < 3; ++i) {
    mips[i] = vxb_range_mipmap(g, i);
    vxb_range_mipmap_stride(g, i, ms[i]);
  }
  return vx_upload_volume(c, vxb_indirection_data(g), is, vxb_range_data(g), rs, vxb_atlas_data(g), as, 3, mips,
                          ms, ext);
}

int vx_set_layout(VxContext* c, int layout) {
  if (!c) return VX_ERR_INVALID;
  if (is_group(c)) return fan_out(c, [&](VxContext* m, size_t) { return vx_set_layout(m, layout); });
  VX_DEV(c);
  if (layout != VX_LAYOUT_REFERENCE && layout != VX_LAYOUT_CELLQUAD && layout != VX_LAYOUT_BRICKF32 &&
      layout != VX_LAYOUT_AUTO && layout != VX_LAYOUT_BRICKU8)
    VX_FAIL(c, VX_ERR_INVALID, "vx_set_layout: unknown layout %d", layout);
  if (layout == c->layout) return VX_OK;
  c->layout = layout;
  if (c->vol.has_volume) {
    VX_HIP(c, hipStreamSynchronize(c->stream));
    reset_layouts(c);
    if (int rc = build_one_layout(c, primary_layout(c))) return rc;
    VX_HIP(c, hipStreamSynchronize(c->stream));
  }
  return VX_OK;
}

}  // extern "C"
