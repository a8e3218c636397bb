/*
 * volxel_napi.c -- thin Node N-API shim over the C ABI of libvolxel_hip.so
 * (include/volxel_hip.h, include/volxel_brick.h).  One JS function per C entry point;
 * typed arrays are passed without copying; a non-zero status becomes a thrown JS Error
 * carrying vx_last_error(), so the host's handleError contract (viewer.ts:797-816) holds.
 * Plain C against <node_api.h> (N-API v3+, Node >= 10).
 *
 * The helpers come first: arguments in (the context handle among them) and results out in volxel_napi_helpers.h, shared with
 * the addons of the distance calls and of the segment store (volxel_napi_distance.c, volxel_napi_segments.c); grids out and the making of context handles below.  A wrapper
 * states only what is particular to its entry point: it opens with CTX_ARGS (or get_args where there is no context), reads a
 * params struct with struct_arg and a typed array with typed / typed_or_null / typed_required, and answers with status,
 * num_object or the set_* calls.  A new wrapper is written from these, not from a neighbour.
 */
#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/volxel_brick.h"
#include "../../include/volxel_hip.h"

#include "volxel_napi_helpers.h"

static napi_value make_typed(napi_env env, napi_typedarray_type t, const void* src, size_t count, size_t esz) {
  napi_value ab, ta;
  void* dst = NULL;
  if (napi_create_arraybuffer(env, count * esz, &dst, &ab) != napi_ok) return NULL;
  if (count) memcpy(dst, src, count * esz);
  if (napi_create_typedarray(env, t, count, ab, 0, &ta) != napi_ok) return NULL;
  return ta;
}

static void set_pair(napi_env env, napi_value o, const char* name, napi_value x, napi_value y) {
  napi_value pair;
  napi_create_array_with_length(env, 2, &pair);
  napi_set_element(env, pair, 0, x);
  napi_set_element(env, pair, 1, y);
  napi_set_named_property(env, o, name, pair);
}

/* a built grid -> WasmWorkerMessageDicomReturn-shaped object (worker.ts:19-58 copies every buffer out and frees the
 * grid; so does this) */
static napi_value grid_to_object(napi_env env, VxBrickGrid* g) {
  uint32_t is[3], rs[3], as[3], ext[3];
  vxb_indirection_size(g, is);
  vxb_range_size(g, rs);
  vxb_atlas_size(g, as);
  vxb_index_extent(g, ext);
  size_t nb = (size_t)is[0] * is[1] * is[2];
  napi_value o, v, e;
  napi_create_object(env, &o);
  napi_create_string_utf8(env, "return_dicom", NAPI_AUTO_LENGTH, &v);
  napi_set_named_property(env, o, "type", v);
  set_u3(env, o, "indirectionSize", is);
  set_u3(env, o, "rangeSize", rs);
  set_u3(env, o, "atlasSize", as);
  set_u3(env, o, "indexExtent", ext);
  napi_set_named_property(env, o, "indirection", make_typed(env, napi_uint32_array, vxb_indirection_data(g), nb, 4));
  napi_set_named_property(env, o, "range", make_typed(env, napi_uint16_array, vxb_range_data(g), nb * 2, 2));
  napi_set_named_property(env, o, "atlas",
                          make_typed(env, napi_uint8_array, vxb_atlas_data(g), (size_t)as[0] * as[1] * as[2], 1));
  float t[16];
  vxb_transform(g, t);
  napi_set_named_property(env, o, "transform", make_typed(env, napi_float32_array, t, 16, 4));
  uint32_t hl = vxb_histogram_len(g);
  napi_set_named_property(env, o, "histogram", make_typed(env, napi_uint32_array, vxb_histogram(g), hl, 4));
  napi_set_named_property(env, o, "histogramGradient",
                          make_typed(env, napi_int32_array, vxb_histogram_gradient(g), hl, 4));
  napi_create_uint32(env, vxb_histogram_gradient_min(g), &v);
  napi_create_uint32(env, vxb_histogram_gradient_max(g), &e);
  set_pair(env, o, "histogramGradientRange", v, e);
  napi_create_double(env, vxb_minorant(g), &v);
  napi_create_double(env, vxb_majorant(g), &e);
  set_pair(env, o, "minMaj", v, e);
  napi_value mips;
  uint32_t nm = vxb_range_mipmaps(g);
  napi_create_array_with_length(env, nm, &mips);
  for (uint32_t k = 0; k < nm; ++k) {
    uint32_t st[3];
    vxb_range_mipmap_stride(g, k, st);
    napi_value mo;
    napi_create_object(env, &mo);
    napi_set_named_property(env, mo, "mipmap",
                            make_typed(env, napi_uint16_array, vxb_range_mipmap(g, k), (size_t)st[0] * st[1] * st[2] * 2, 2));
    set_u3(env, mo, "stride", st);
    napi_set_element(env, mips, k, mo);
  }
  napi_set_named_property(env, o, "rangeMipmaps", mips);
  napi_create_uint32(env, vxb_brick_counter(g), &e);
  napi_set_named_property(env, o, "brickCounter", e);
  vxb_free(g); /* worker.ts:54 */
  return o;
}

/* ---- context handles ------------------------------------------------------------------------------------------------ */
static void ctx_finalize(napi_env env, void* data, void* hint) {
  (void)env; (void)hint;
  Handle* h = (Handle*)data;
  if (!h) return;
  if (h->ctx) vx_destroy(h->ctx); /* a handle dropped without destroy() still releases the device memory */
  free(h);
}

/* a created context -> JS handle (the context is destroyed if wrapping fails) */
static napi_value wrap_ctx(napi_env env, VxContext* c) {
  Handle* box = (Handle*)malloc(sizeof(Handle));
  if (!box) {
    vx_destroy(c);
    return throw_msg(env, "volxel_napi: out of memory");
  }
  box->ctx = c;
  napi_value h;
  if (napi_create_external(env, box, ctx_finalize, NULL, &h) != napi_ok) {
    vx_destroy(c);
    free(box);
    return throw_msg(env, "volxel_napi: napi_create_external failed");
  }
  return h;
}

/* ---- the entry points ----------------------------------------------------------------------------------------------- */
/* create(deviceId) -> handle */
static napi_value n_create(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  int32_t dev = 0;
  NAPI_OK(napi_get_value_int32(env, a[0], &dev));
  VxContext* c = NULL;
  if (vx_create(dev, &c) != VX_OK) return throw_msg(env, vx_last_error(NULL));
  return wrap_ctx(env, c);
}

/* createGroup([deviceId, ...]) -> handle of a device group (vx_create_group: member i renders shard i) */
static napi_value n_create_group(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  bool is_array = false;
  uint32_t n = 0;
  if (napi_is_array(env, a[0], &is_array) != napi_ok || !is_array || napi_get_array_length(env, a[0], &n) != napi_ok ||
      n < 1 || n > VX_GROUP_MAX) {
    napi_throw_type_error(env, NULL, "volxel_napi: createGroup expects an array of 1 to 64 device ids");
    return NULL;
  }
  int ids[VX_GROUP_MAX];
  for (uint32_t i = 0; i < n; ++i) {
    napi_value e;
    int32_t d = 0;
    if (napi_get_element(env, a[0], i, &e) != napi_ok || napi_get_value_int32(env, e, &d) != napi_ok) {
      napi_throw_type_error(env, NULL, "volxel_napi: createGroup expects integer device ids");
      return NULL;
    }
    ids[i] = d;
  }
  VxContext* c = NULL;
  if (vx_create_group(ids, (int)n, &c) != VX_OK) return throw_msg(env, vx_last_error(NULL));
  return wrap_ctx(env, c);
}

/* destroy(handle): idempotent */
static napi_value n_destroy(napi_env env, napi_callback_info info) {
  napi_value a[1];
  if (!get_args(env, info, 1, a)) return NULL;
  Handle* h = get_handle(env, a[0]);
  if (!h) return NULL;
  if (h->ctx) vx_destroy(h->ctx);
  h->ctx = NULL;
  return NULL;
}

/* uploadVolume(ctx, msg): msg = WasmWorkerMessageDicomReturn (common.ts:37-55) */
static napi_value n_upload_volume(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  napi_value m = a[1];
  void *ind, *rng, *atl;
  size_t n, n_ind, n_rng, n_atl;
  uint32_t is[3], rs[3], as[3], ext[3];
  if (!typed(env, prop(env, m, "indirection"), napi_uint32_array, &ind, &n_ind)) return NULL;
  if (!typed(env, prop(env, m, "range"), napi_uint16_array, &rng, &n_rng)) return NULL;
  if (!typed(env, prop(env, m, "atlas"), napi_uint8_array, &atl, &n_atl)) return NULL;
  if (!u32x3(env, prop(env, m, "indirectionSize"), is) || !u32x3(env, prop(env, m, "rangeSize"), rs) ||
      !u32x3(env, prop(env, m, "atlasSize"), as) || !u32x3(env, prop(env, m, "indexExtent"), ext))
    return NULL;
  /* the C ABI takes raw pointers: the typed arrays must really hold what the size fields promise */
  if ((uint64_t)n_ind < prod3(is)) return throw_msg(env, "uploadVolume: indirection shorter than indirectionSize");
  if ((uint64_t)n_rng < 2u * prod3(rs)) return throw_msg(env, "uploadVolume: range shorter than 2 * rangeSize");
  if ((uint64_t)n_atl < prod3(as)) return throw_msg(env, "uploadVolume: atlas shorter than atlasSize");
  napi_value mips = prop(env, m, "rangeMipmaps");
  uint32_t nm = 0;
  NAPI_OK(napi_get_array_length(env, mips, &nm));
  const uint16_t* mp[3] = {0, 0, 0};
  uint32_t ms[3][3];
  if (nm > 3) nm = 3;
  for (uint32_t k = 0; k < nm; ++k) {
    napi_value e;
    void* d;
    NAPI_OK(napi_get_element(env, mips, k, &e));
    if (!typed(env, prop(env, e, "mipmap"), napi_uint16_array, &d, &n)) return NULL;
    mp[k] = (const uint16_t*)d;
    if (!u32x3(env, prop(env, e, "stride"), ms[k])) return NULL;
    if ((uint64_t)n < 2u * prod3(ms[k])) return throw_msg(env, "uploadVolume: range mipmap shorter than 2 * stride");
  }
  return status(env, c, vx_upload_volume(c, (const uint32_t*)ind, is, (const uint16_t*)rng, rs, (const uint8_t*)atl, as, (int)nm,
                                         mp, (const uint32_t(*)[3])ms, ext));
}

static napi_value n_upload_transfer(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  void* d;
  size_t n;
  uint32_t len;
  if (!typed(env, a[1], napi_float32_array, &d, &n)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &len));
  if (n < (size_t)len * 4) return throw_msg(env, "uploadTransfer: data shorter than length*4");
  return status(env, c, vx_upload_transfer(c, (const float*)d, len));
}

/* uploadEnvironment(ctx, Float32Array rgba | null, width, height): `new Environment(gl, env)` */
static napi_value n_upload_environment(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  if (nullish(env, a[1])) return status(env, c, vx_upload_environment(c, NULL, 0, 0));
  void* d;
  size_t n;
  uint32_t w, h;
  if (!typed(env, a[1], napi_float32_array, &d, &n)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &w));
  NAPI_OK(napi_get_value_uint32(env, a[3], &h));
  if (n < (size_t)w * h * 4) return throw_msg(env, "uploadEnvironment: data shorter than width*height*4");
  return status(env, c, vx_upload_environment(c, (const float*)d, w, h));
}

/* setParams(ctx, ArrayBuffer holding one VxParams) */
static napi_value n_set_params(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  VxParams p;
  if (!struct_arg(env, a[1], &p, sizeof p, "setParams", "VxParams")) return NULL;
  return status(env, c, vx_set_params(c, &p));
}

/* sizeofParams(), sizeofSliceParams(), sizeofIsoParams(), sizeofSegmentParams(), sizeofMeshParams(): one callback; init
 * binds each export's size as the function's data */
static napi_value n_sizeof(napi_env env, napi_callback_info info) {
  void* size = NULL;
  napi_value v;
  NAPI_OK(napi_get_cb_info(env, info, NULL, NULL, NULL, &size));
  NAPI_OK(napi_create_uint32(env, (uint32_t)(uintptr_t)size, &v));
  return v;
}

static napi_value n_resize(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  uint32_t w, h;
  NAPI_OK(napi_get_value_uint32(env, a[1], &w));
  NAPI_OK(napi_get_value_uint32(env, a[2], &h));
  return status(env, c, vx_resize(c, w, h));
}

static napi_value n_set_layout(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  int32_t l;
  NAPI_OK(napi_get_value_int32(env, a[1], &l));
  return status(env, c, vx_set_layout(c, l));
}

static napi_value n_render_frame(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  uint32_t f;
  double w;
  NAPI_OK(napi_get_value_uint32(env, a[1], &f));
  NAPI_OK(napi_get_value_double(env, a[2], &w));
  return status(env, c, vx_render_frame(c, f, (float)w));
}

/* renderFrames(ctx, firstFrame, Float32Array weights, inFlight): weights.length accumulation frames,
 * up to inFlight of them per launch (vx_render_frames) */
static napi_value n_render_frames(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  uint32_t f;
  int32_t in_flight;
  void* w;
  size_t n;
  NAPI_OK(napi_get_value_uint32(env, a[1], &f));
  if (!typed(env, a[2], napi_float32_array, &w, &n)) return NULL;
  NAPI_OK(napi_get_value_int32(env, a[3], &in_flight));
  if (n > 0xffffffffu) return throw_msg(env, "renderFrames: too many frames");
  return status(env, c, vx_render_frames(c, f, (uint32_t)n, (const float*)w, in_flight));
}

/* probeTileCosts(ctx, Uint32Array out): cost estimate of every 64x64 tile (vx_probe_tile_costs) */
static napi_value n_probe_tile_costs(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* d;
  size_t n;
  if (!typed(env, a[1], napi_uint32_array, &d, &n)) return NULL;
  return status(env, c, vx_probe_tile_costs(c, (uint32_t*)d, (uint32_t)n));
}

/* setTileOrder(ctx, Uint32Array perm | null): dealing order of the tiles over the shards (vx_set_tile_order) */
static napi_value n_set_tile_order(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* d;
  size_t n;
  if (!typed_or_null(env, a[1], napi_uint32_array, &d, &n)) return NULL;
  return status(env, c, vx_set_tile_order(c, (const uint32_t*)d, (uint32_t)n));
}

/* deviceInfo(ctx) -> { name, computeUnits, hbmBytes } */
static napi_value n_device_info(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  char name[256];
  uint32_t cus = 0;
  uint64_t hbm = 0;
  if (vx_device_info(c, name, sizeof name, &cus, &hbm) != VX_OK) return throw_msg(env, vx_last_error(c));
  napi_value o, v;
  if (napi_create_object(env, &o) != napi_ok || napi_create_string_utf8(env, name, NAPI_AUTO_LENGTH, &v) != napi_ok ||
      napi_set_named_property(env, o, "name", v) != napi_ok || !set_num(env, o, "computeUnits", cus) ||
      !set_num(env, o, "hbmBytes", (double)hbm))
    return throw_result(env, "deviceInfo");
  return o;
}

static napi_value n_finish(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  return status(env, c, vx_finish(c));
}

static napi_value n_read_accum(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* d;
  size_t n;
  uint32_t w = 0, h = 0;
  if (!typed(env, a[1], napi_float32_array, &d, &n)) return NULL;
  vx_render_size(c, &w, &h);
  if (n < (size_t)w * h * 4) return throw_msg(env, "readAccum: buffer smaller than width*height*4 floats");
  return status(env, c, vx_read_accum(c, (float*)d));
}

static napi_value n_read_display(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  void* d;
  size_t n;
  double ex, ga;
  if (!typed(env, a[1], napi_uint8_array, &d, &n)) return NULL;
  NAPI_OK(napi_get_value_double(env, a[2], &ex));
  NAPI_OK(napi_get_value_double(env, a[3], &ga));
  uint32_t w = 0, h = 0;
  vx_render_size(c, &w, &h);
  if (n < (size_t)w * h * 4) return throw_msg(env, "readDisplay: buffer smaller than width*height*4 bytes");
  return status(env, c, vx_read_display(c, (uint8_t*)d, (float)ex, (float)ga));
}

/* readDisplayScaled(ctx, Uint8Array out, outW, outH, exposure, gamma): the blit to a canvas */
static napi_value n_read_display_scaled(napi_env env, napi_callback_info info) {
  CTX_ARGS(6);
  void* d;
  size_t n;
  uint32_t ow, oh;
  double ex, ga;
  if (!typed(env, a[1], napi_uint8_array, &d, &n)) return NULL;
  NAPI_OK(napi_get_value_uint32(env, a[2], &ow));
  NAPI_OK(napi_get_value_uint32(env, a[3], &oh));
  NAPI_OK(napi_get_value_double(env, a[4], &ex));
  NAPI_OK(napi_get_value_double(env, a[5], &ga));
  if (n < (size_t)ow * oh * 4) return throw_msg(env, "readDisplayScaled: buffer smaller than outW*outH*4 bytes");
  return status(env, c, vx_read_display_scaled(c, (uint8_t*)d, ow, oh, (float)ex, (float)ga));
}

static napi_value n_get_counters(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  VxCounters k;
  if (vx_get_counters(c, &k) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"samples", (double)k.samples}, {"rays", (double)k.rays}, {"pixels", (double)k.pixels},
                   {"skipSteps", (double)k.skip_steps}, {"gradSamples", (double)k.grad_samples},
                   {"tfSamples", (double)k.tf_samples}, {"activeLaneSlots", (double)k.active_lane_slots},
                   {"laneSlots", (double)k.lane_slots}, {"launches", (double)k.launches}, {"frames", (double)k.frames},
                   {"kernelMs", (double)k.kernel_ms}, {"lastKernelMs", (double)k.last_kernel_ms},
                   {"gathers", (double)k.gathers}, {"ldsReads", (double)k.lds_reads}, {"mergeMs", (double)k.merge_ms},
                   {"minLaunchFrames", (double)k.min_launch_frames}, {"maxLaunchFrames", (double)k.max_launch_frames},
                   {"mergeLaunches", (double)k.merge_launches}};
  return num_object(env, "getCounters", f, COUNT(f));
}

static napi_value n_reset_counters(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  return status(env, c, vx_reset_counters(c));
}

/* shadowStats(ctx) -> { builds, lightSamples, lastBuildMs } (vx_shadow_stats) */
static napi_value n_shadow_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint64_t builds = 0, samples = 0;
  double ms = 0.0;
  if (vx_shadow_stats(c, &builds, &samples, &ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"builds", (double)builds}, {"lightSamples", (double)samples}, {"lastBuildMs", ms}};
  return num_object(env, "shadowStats", f, COUNT(f));
}

/* readShadowGrid(ctx) -> { dims: [nx, ny, nz], data: Float32Array } (vx_debug_read_shadow_grid) */
static napi_value n_read_shadow_grid(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t dims[3];
  if (vx_debug_read_shadow_grid(c, NULL, dims) != VX_OK) return throw_msg(env, vx_last_error(c));
  const size_t n = (size_t)dims[0] * dims[1] * dims[2];
  napi_value ab, arr, o;
  void* data = NULL;
  NAPI_OK(napi_create_arraybuffer(env, n * sizeof(float), &data, &ab));
  if (vx_debug_read_shadow_grid(c, (float*)data, dims) != VX_OK) return throw_msg(env, vx_last_error(c));
  NAPI_OK(napi_create_typedarray(env, napi_float32_array, n, ab, 0, &arr));
  NAPI_OK(napi_create_object(env, &o));
  if (!set_u3(env, o, "dims", dims)) return throw_result(env, "readShadowGrid");
  NAPI_OK(napi_set_named_property(env, o, "data", arr));
  return o;
}

/* slice(ctx, ArrayBuffer holding one VxSliceParams, Float32Array | null values, Uint8Array | null rgba8) (vx_slice) */
static napi_value n_slice(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  VxSliceParams sp;
  if (!struct_arg(env, a[1], &sp, sizeof sp, "slice", "VxSliceParams")) return NULL;
  void *vals, *rgba;
  size_t nv, nr;
  if (!typed_or_null(env, a[2], napi_float32_array, &vals, &nv)) return NULL;
  if (!typed_or_null(env, a[3], napi_uint8_array, &rgba, &nr)) return NULL;
  const size_t px = (size_t)sp.size[0] * sp.size[1];
  if (vals && nv < px) return throw_msg(env, "slice: values shorter than size[0]*size[1] floats");
  if (rgba && nr < px * 4) return throw_msg(env, "slice: rgba8 shorter than size[0]*size[1]*4 bytes");
  return status(env, c, vx_slice(c, &sp, (float*)vals, (uint8_t*)rgba));
}

/* sliceStats(ctx) -> { samples, lastKernelMs } (vx_slice_stats) */
static napi_value n_slice_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint64_t samples = 0;
  double ms = 0.0;
  if (vx_slice_stats(c, &samples, &ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"samples", (double)samples}, {"lastKernelMs", ms}};
  return num_object(env, "sliceStats", f, COUNT(f));
}

/* isosurface(ctx, ArrayBuffer holding one VxIsoParams, Float32Array | null rgba, Float32Array | null hit) (vx_isosurface); the
 * arrays hold 4 floats per pixel of the window (ip.window; all zero: the whole render size) */
static napi_value n_isosurface(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  VxIsoParams ip;
  if (!struct_arg(env, a[1], &ip, sizeof ip, "isosurface", "VxIsoParams")) return NULL;
  void *rgba, *hit;
  size_t nr, nh;
  if (!typed_or_null(env, a[2], napi_float32_array, &rgba, &nr)) return NULL;
  if (!typed_or_null(env, a[3], napi_float32_array, &hit, &nh)) return NULL;
  if (ip.window[2] <= ip.window[0] || ip.window[3] <= ip.window[1])
    return throw_msg(env, "isosurface: the host passes an explicit window (x0 < x1, y0 < y1)");
  const size_t px = (size_t)(ip.window[2] - ip.window[0]) * (ip.window[3] - ip.window[1]);
  if (rgba && nr < px * 4) return throw_msg(env, "isosurface: rgba shorter than 4 floats per window pixel");
  if (hit && nh < px * 4) return throw_msg(env, "isosurface: hit shorter than 4 floats per window pixel");
  return status(env, c, vx_isosurface(c, &ip, (float*)rgba, (float*)hit));
}

/* isoStats(ctx) -> { rays, hits, samples, refineSamples, skipped, lastKernelMs } (vx_iso_stats) */
static napi_value n_iso_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint64_t v[5] = {0, 0, 0, 0, 0};
  double ms = 0.0;
  if (vx_iso_stats(c, &v[0], &v[1], &v[2], &v[3], &v[4], &ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"rays", (double)v[0]}, {"hits", (double)v[1]}, {"samples", (double)v[2]}, {"refineSamples", (double)v[3]},
                   {"skipped", (double)v[4]}, {"lastKernelMs", ms}};
  return num_object(env, "isoStats", f, COUNT(f));
}

/* segment(ctx, ArrayBuffer holding one VxSegmentParams) -> { count, bboxLo, bboxHi, dMin, dMax, dSum, rounds, converged,
 * brickVisits } (vx_segment) */
static napi_value n_segment(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  VxSegmentParams sp;
  if (!struct_arg(env, a[1], &sp, sizeof sp, "segment", "VxSegmentParams")) return NULL;
  VxSegmentResult r;
  if (vx_segment(c, &sp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* segmentThreshold(ctx, ArrayBuffer holding one VxSegmentParams) -> what segment returns, for the whole band (vx_segment_threshold) */
static napi_value n_segment_threshold(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  VxSegmentParams sp;
  if (!struct_arg(env, a[1], &sp, sizeof sp, "threshold", "VxSegmentParams")) return NULL;
  VxSegmentResult r;
  if (vx_segment_threshold(c, &sp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* segmentEdit(ctx, op 0 .. 4, connectivity, steps, band 0 | 1) -> what segment returns, for the edited mask (vx_segment_edit) */
static napi_value n_segment_edit(napi_env env, napi_callback_info info) {
  CTX_ARGS(5);
  int32_t op, conn, band;
  uint32_t steps;
  if (napi_get_value_int32(env, a[1], &op) != napi_ok || napi_get_value_int32(env, a[2], &conn) != napi_ok ||
      napi_get_value_uint32(env, a[3], &steps) != napi_ok || napi_get_value_int32(env, a[4], &band) != napi_ok)
    return throw_msg(env, "segmentEdit: op, connectivity, steps and band must be numbers");
  VxSegmentEditParams ep = {op, conn, steps, band};
  VxSegmentResult r;
  if (vx_segment_edit(c, &ep, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* setSegmentMask(ctx, Uint8Array of X*Y*Z/8 bytes) -> what segment returns, for the installed mask (vx_segment_write_mask) */
static napi_value n_set_segment_mask(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* bits;
  size_t nb;
  if (!typed_required(env, a[1], napi_uint8_array, "setSegmentMask: bits must be a Uint8Array", &bits, &nb)) return NULL;
  VxSegmentResult r;
  if (vx_segment_write_mask(c, (const uint8_t*)bits, (uint64_t)nb, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* segmentEditStats(ctx) -> { launches, editMs, statsMs } (vx_segment_edit_stats) */
static napi_value n_segment_edit_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t launches = 0;
  double ms[2] = {0.0, 0.0};
  if (vx_segment_edit_stats(c, &launches, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"launches", launches}, {"editMs", ms[0]}, {"statsMs", ms[1]}};
  return num_object(env, "segmentEditStats", f, COUNT(f));
}

/* segmentIslands(ctx, op 0 .. 3, connectivity, keep, minVoxels, sx, sy, sz) -> { islands, kept, largest, seg: what segment
 * returns, for the mask after the op } (vx_segment_islands; counts up to 2^53 as doubles) */
static napi_value n_segment_islands(napi_env env, napi_callback_info info) {
  CTX_ARGS(8);
  int32_t op, conn;
  double keep, minv;
  uint32_t sd[3];
  if (napi_get_value_int32(env, a[1], &op) != napi_ok || napi_get_value_int32(env, a[2], &conn) != napi_ok ||
      napi_get_value_double(env, a[3], &keep) != napi_ok || napi_get_value_double(env, a[4], &minv) != napi_ok ||
      napi_get_value_uint32(env, a[5], &sd[0]) != napi_ok || napi_get_value_uint32(env, a[6], &sd[1]) != napi_ok ||
      napi_get_value_uint32(env, a[7], &sd[2]) != napi_ok || !(keep >= 0.0) || !(minv >= 0.0))
    return throw_msg(env, "segmentIslands: op, connectivity, keep, minVoxels and the seed must be numbers >= 0");
  VxIslandsParams ip = {op, conn, (uint64_t)keep, (uint64_t)minv, {sd[0], sd[1], sd[2]}, 0u};
  VxIslandsResult r;
  if (vx_segment_islands(c, &ip, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  napi_value seg = segment_result(env, &r.seg);
  if (!seg) return NULL;
  const Num f[] = {{"islands", (double)r.islands}, {"kept", (double)r.kept}, {"largest", (double)r.largest}};
  napi_value o = num_object(env, "segmentIslands", f, COUNT(f));
  if (o && napi_set_named_property(env, o, "seg", seg) != napi_ok) return throw_result(env, "segmentIslands");
  return o;
}

/* rows -> [{ label, count, anchor, bboxLo, bboxHi }], or NULL when a step failed */
static napi_value islands_table(napi_env env, const VxIsland* rows, size_t cnt) {
  napi_value arr, o;
  if (napi_create_array_with_length(env, cnt, &arr) != napi_ok) return NULL;
  for (size_t i = 0; i < cnt; ++i)
    if (napi_create_object(env, &o) != napi_ok || !set_num(env, o, "label", rows[i].label) ||
        !set_num(env, o, "count", (double)rows[i].count) || !set_u3(env, o, "anchor", rows[i].anchor) ||
        !set_u3(env, o, "bboxLo", rows[i].bbox_lo) || !set_u3(env, o, "bboxHi", rows[i].bbox_hi) ||
        napi_set_element(env, arr, (uint32_t)i, o) != napi_ok)
      return NULL;
  return arr;
}

/* islandsRead(ctx, first, n) -> the rows first .. first + n - 1 of the island table (vx_islands_read) */
static napi_value n_islands_read(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  double first, n;
  if (napi_get_value_double(env, a[1], &first) != napi_ok || napi_get_value_double(env, a[2], &n) != napi_ok || !(first >= 0.0) ||
      !(n >= 0.0) || n > 268435456.0)
    return throw_msg(env, "islandsRead: first and n must be numbers >= 0 (n <= 2^28)");
  const size_t cnt = (size_t)n;
  VxIsland* rows = (VxIsland*)malloc((cnt ? cnt : 1) * sizeof(VxIsland));
  if (!rows) return throw_msg(env, "islandsRead: out of memory");
  napi_value out;
  if (vx_islands_read(c, (uint64_t)first, (uint64_t)cnt, rows) != VX_OK) out = throw_msg(env, vx_last_error(c));
  else if (!(out = islands_table(env, rows, cnt))) out = throw_result(env, "islandsRead");
  free(rows);
  return out;
}

/* islandsReadLabels(ctx, Uint32Array of X*Y*Z labels) (vx_islands_read_labels) */
static napi_value n_islands_read_labels(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* out;
  size_t n;
  if (!typed_required(env, a[1], napi_uint32_array, "islandsReadLabels: labels must be a Uint32Array", &out, &n)) return NULL;
  return status(env, c, vx_islands_read_labels(c, (uint32_t*)out, (uint64_t)n));
}

/* islandsStats(ctx) -> { launches, localMs, mergeMs, flattenMs, tableMs, hostRankMs, applyMs, statsMs } (vx_islands_stats) */
static napi_value n_islands_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t launches = 0;
  double ms[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  if (vx_islands_stats(c, &launches, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"launches", launches}, {"localMs", ms[0]}, {"mergeMs", ms[1]}, {"flattenMs", ms[2]}, {"tableMs", ms[3]},
                   {"hostRankMs", ms[4]}, {"applyMs", ms[5]}, {"statsMs", ms[6]}};
  return num_object(env, "islandsStats", f, COUNT(f));
}

/* meshExtract(ctx, ArrayBuffer holding one VxMeshParams) -> { vertices, triangles, activeBlocks, blocks, bboxLo, bboxHi }
 * (vx_mesh_extract; the bbox components are cells, -1 included) */
static napi_value n_mesh_extract(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  VxMeshParams mp;
  if (!struct_arg(env, a[1], &mp, sizeof mp, "extractMesh", "VxMeshParams")) return NULL;
  VxMeshResult r;
  if (vx_mesh_extract(c, &mp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"vertices", (double)r.vertices}, {"triangles", (double)r.triangles},
                   {"activeBlocks", (double)r.active_blocks}, {"blocks", (double)r.blocks}};
  napi_value o = num_object(env, "extractMesh", f, COUNT(f));
  if (o && (!set_x3(env, o, "bboxLo", r.bbox_lo, 1) || !set_x3(env, o, "bboxHi", r.bbox_hi, 1)))
    return throw_result(env, "extractMesh");
  return o;
}

/* meshRead(ctx, Float32Array of 3 * vertices, Int32Array of 3 * vertices, Uint32Array of 3 * triangles) (vx_mesh_read); the
 * lengths are those meshExtract returned -- viewer.js allocates them from its result */
static napi_value n_mesh_read(napi_env env, napi_callback_info info) {
  CTX_ARGS(4);
  void *v, *ce, *t;
  size_t nv, nc, nt;
  if (!typed_or_null(env, a[1], napi_float32_array, &v, &nv) || !typed_or_null(env, a[2], napi_int32_array, &ce, &nc) ||
      !typed_or_null(env, a[3], napi_uint32_array, &t, &nt))
    return NULL;
  return status(env, c, vx_mesh_read(c, (float*)v, (int32_t*)ce, (uint32_t*)t));
}

/* meshStats(ctx) -> { launches, insideMs, activeMs, emitMs } (vx_mesh_stats) */
static napi_value n_mesh_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t launches = 0;
  double ms[3] = {0.0, 0.0, 0.0};
  if (vx_mesh_stats(c, &launches, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"launches", launches}, {"insideMs", ms[0]}, {"activeMs", ms[1]}, {"emitMs", ms[2]}};
  return num_object(env, "meshStats", f, COUNT(f));
}

/* segmentMask(ctx, Uint8Array of X*Y*Z/8 bytes) (vx_segment_read_mask) */
static napi_value n_segment_mask(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* bits;
  size_t nb;
  if (!typed_required(env, a[1], napi_uint8_array, "segmentMask: bits must be a Uint8Array", &bits, &nb)) return NULL;
  return status(env, c, vx_segment_read_mask(c, (uint8_t*)bits, (uint64_t)nb));
}

/* sliceMask(ctx, ArrayBuffer holding one VxSliceParams, Uint8Array of size[0]*size[1] bytes) (vx_slice_segment_mask) */
static napi_value n_slice_mask(napi_env env, napi_callback_info info) {
  static const char too_short[] = "sliceMask: out shorter than size[0]*size[1] bytes";
  CTX_ARGS(3);
  VxSliceParams sp;
  if (!struct_arg(env, a[1], &sp, sizeof sp, "sliceMask", "VxSliceParams")) return NULL;
  void* out;
  size_t no;
  if (!typed_required(env, a[2], napi_uint8_array, too_short, &out, &no)) return NULL;
  if (no < (size_t)sp.size[0] * sp.size[1]) return throw_msg(env, too_short);
  return status(env, c, vx_slice_segment_mask(c, &sp, (uint8_t*)out));
}

/* segmentStats(ctx) -> { rounds, brickVisits, predicateMs, floodMs, statsMs } (vx_segment_stats) */
static napi_value n_segment_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t rounds = 0;
  uint64_t visits = 0;
  double ms[3] = {0.0, 0.0, 0.0};
  if (vx_segment_stats(c, &rounds, &visits, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"rounds", rounds}, {"brickVisits", (double)visits}, {"predicateMs", ms[0]}, {"floodMs", ms[1]},
                   {"statsMs", ms[2]}};
  return num_object(env, "segmentStats", f, COUNT(f));
}

/* setSegmentView(ctx, 0 | 1 | 2) (vx_set_segment_view); getSegmentView(ctx) -> 0 | 1 | 2 (vx_get_segment_view) */
static napi_value n_set_segment_view(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  int32_t view = 0;
  if (napi_get_value_int32(env, a[1], &view) != napi_ok) return throw_msg(env, "setSegmentView: view must be a number");
  return status(env, c, vx_set_segment_view(c, view));
}
static napi_value n_get_segment_view(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  int view = 0;
  if (vx_get_segment_view(c, &view) != VX_OK) return throw_msg(env, vx_last_error(c));
  napi_value v;
  NAPI_OK(napi_create_int32(env, view, &v));
  return v;
}

static napi_value n_version(napi_env env, napi_callback_info info) {
  (void)info;
  napi_value v;
  NAPI_OK(napi_create_string_utf8(env, vx_version(), NAPI_AUTO_LENGTH, &v));
  return v;
}

/* ---- the preprocessor; both calls answer with grid_to_object -------------------------------------------------------- */
/* readDicomsToGrid(Array<Uint8Array> files, threads): the wasm export of lib.rs:193-202 as called
 * at worker.ts:101-104 */
static napi_value n_read_dicoms_to_grid(napi_env env, napi_callback_info info) {
  napi_value a[2];
  if (!get_args(env, info, 2, a)) return NULL;
  uint32_t n = 0, i = 0;
  int32_t threads;
  bool is_arr = false;
  NAPI_OK(napi_is_array(env, a[0], &is_arr));
  if (!is_arr) return throw_msg(env, "readDicomsToGrid: expected an array of Uint8Array");
  NAPI_OK(napi_get_array_length(env, a[0], &n));
  NAPI_OK(napi_get_value_int32(env, a[1], &threads));
  const uint8_t** ptrs = (const uint8_t**)calloc(n ? n : 1, sizeof(*ptrs));
  uint64_t* sizes = (uint64_t*)calloc(n ? n : 1, sizeof(*sizes));
  napi_value out;
  if (!ptrs || !sizes) out = throw_msg(env, "readDicomsToGrid: out of memory");
  else {
    for (; i < n; ++i) {
      napi_value e;
      void* p;
      size_t len;
      if (napi_get_element(env, a[0], i, &e) != napi_ok || !typed(env, e, napi_uint8_array, &p, &len)) break;
      ptrs[i] = (const uint8_t*)p;
      sizes[i] = len;
    }
    VxBrickGrid* g = NULL;
    if (i < n) out = NULL; /* typed() has thrown */
    else if (vxb_read_dicoms_to_grid(ptrs, sizes, n, threads, &g) != VXB_OK) out = throw_msg(env, vxb_last_error());
    else out = grid_to_object(env, g);
  }
  free(ptrs);
  free(sizes);
  return out;
}

/* buildBrickGrid(Uint16Array voxels, [x,y,z], [sx,sy,sz], maxValue, threads) */
static napi_value n_build_brick_grid(napi_env env, napi_callback_info info) {
  napi_value a[5];
  if (!get_args(env, info, 5, a)) return NULL;
  void* vox;
  size_t n;
  uint32_t dims[3], maxv;
  int32_t threads;
  float sp[3];
  if (!typed(env, a[0], napi_uint16_array, &vox, &n) || !u32x3(env, a[1], dims)) return NULL;
  for (uint32_t i = 0; i < 3; ++i) {
    napi_value e;
    double d;
    NAPI_OK(napi_get_element(env, a[2], i, &e));
    NAPI_OK(napi_get_value_double(env, e, &d));
    sp[i] = (float)d;
  }
  NAPI_OK(napi_get_value_uint32(env, a[3], &maxv));
  NAPI_OK(napi_get_value_int32(env, a[4], &threads));
  if (n != (size_t)dims[0] * dims[1] * dims[2]) return throw_msg(env, "buildBrickGrid: voxel count != x*y*z");
  VxBrickGrid* g = NULL;
  if (vxb_build_from_u16((const uint16_t*)vox, dims, sp, (uint16_t)maxv, threads, &g) != VXB_OK)
    return throw_msg(env, vxb_last_error());
  return grid_to_object(env, g);
}

#define SIZEOF(T) n_sizeof, (void*)(uintptr_t)sizeof(T)

static napi_value init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; void* data; } fns[] = {
      {"create", n_create}, {"createGroup", n_create_group}, {"destroy", n_destroy}, {"uploadVolume", n_upload_volume},
      {"uploadTransfer", n_upload_transfer}, {"uploadEnvironment", n_upload_environment}, {"setParams", n_set_params},
      {"sizeofParams", SIZEOF(VxParams)}, {"resize", n_resize}, {"setLayout", n_set_layout}, {"renderFrame", n_render_frame},
      {"renderFrames", n_render_frames}, {"probeTileCosts", n_probe_tile_costs}, {"setTileOrder", n_set_tile_order},
      {"deviceInfo", n_device_info}, {"finish", n_finish}, {"readAccum", n_read_accum}, {"readDisplay", n_read_display},
      {"readDisplayScaled", n_read_display_scaled}, {"getCounters", n_get_counters},
      {"resetCounters", n_reset_counters}, {"shadowStats", n_shadow_stats}, {"readShadowGrid", n_read_shadow_grid},
      {"slice", n_slice}, {"sliceStats", n_slice_stats}, {"sizeofSliceParams", SIZEOF(VxSliceParams)},
      {"isosurface", n_isosurface}, {"isoStats", n_iso_stats}, {"sizeofIsoParams", SIZEOF(VxIsoParams)},
      {"segment", n_segment}, {"sizeofSegmentParams", SIZEOF(VxSegmentParams)}, {"segmentMask", n_segment_mask},
      {"sliceMask", n_slice_mask}, {"segmentStats", n_segment_stats}, {"setSegmentView", n_set_segment_view},
      {"getSegmentView", n_get_segment_view}, {"segmentEdit", n_segment_edit}, {"setSegmentMask", n_set_segment_mask},
      {"segmentEditStats", n_segment_edit_stats},
      {"segmentThreshold", n_segment_threshold}, {"segmentIslands", n_segment_islands}, {"islandsRead", n_islands_read},
      {"islandsReadLabels", n_islands_read_labels}, {"islandsStats", n_islands_stats},
      {"meshExtract", n_mesh_extract}, {"sizeofMeshParams", SIZEOF(VxMeshParams)}, {"meshRead", n_mesh_read},
      {"meshStats", n_mesh_stats},
      {"version", n_version}, {"buildBrickGrid", n_build_brick_grid},
      {"readDicomsToGrid", n_read_dicoms_to_grid}};
  for (size_t i = 0; i < COUNT(fns); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, fns[i].data, &f) != napi_ok ||
        napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
      napi_throw_error(env, NULL, "volxel_napi: export failed");
      return NULL;
    }
  }
  return exports;
}

NAPI_MODULE(volxel_napi, init)
