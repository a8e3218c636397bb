/*
 * volxel_napi_segments.c -- the N-API addon of the segment store (vx_segment_store, vx_segment_load, vx_segment_drop,
 * vx_segment_slots, vx_segment_combine, vx_segment_compare, vx_segments_labelmap; include/volxel_hip.h "the segment store"):
 * volxel_napi_segments.node, beside volxel_napi.node and volxel_napi_distance.node and written from the same helpers
 * (volxel_napi_helpers.h).  Every function takes a context handle made by volxel_napi.node's create.
 */
#include "volxel_napi_helpers.h"

/* storeSegment(ctx, slot) (vx_segment_store) */
static napi_value n_store_segment(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  uint32_t slot;
  if (napi_get_value_uint32(env, a[1], &slot) != napi_ok) return throw_msg(env, "storeSegment: slot must be a number");
  return status(env, c, vx_segment_store(c, slot));
}

/* loadSegment(ctx, slot) -> what segment returns, for the slot's mask (vx_segment_load) */
static napi_value n_load_segment(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  uint32_t slot;
  if (napi_get_value_uint32(env, a[1], &slot) != napi_ok) return throw_msg(env, "loadSegment: slot must be a number");
  VxSegmentResult r;
  if (vx_segment_load(c, slot, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* dropSegment(ctx, slot) (vx_segment_drop) */
static napi_value n_drop_segment(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  uint32_t slot;
  if (napi_get_value_uint32(env, a[1], &slot) != napi_ok) return throw_msg(env, "dropSegment: slot must be a number");
  return status(env, c, vx_segment_drop(c, slot));
}

/* storedSegments(ctx) -> the occupied bits as a number (vx_segment_slots) */
static napi_value n_stored_segments(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t bits = 0;
  napi_value v;
  if (vx_segment_slots(c, &bits) != VX_OK) return throw_msg(env, vx_last_error(c));
  NAPI_OK(napi_create_uint32(env, bits, &v));
  return v;
}

/* segmentCombine(ctx, op 0 .. 4, slot) -> what segment returns, for the new mask (vx_segment_combine) */
static napi_value n_segment_combine(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  int32_t op;
  uint32_t slot;
  if (napi_get_value_int32(env, a[1], &op) != napi_ok || napi_get_value_uint32(env, a[2], &slot) != napi_ok)
    return throw_msg(env, "segmentCombine: op and slot must be numbers");
  VxCombineParams cp = {op, slot};
  VxSegmentResult r;
  if (vx_segment_combine(c, &cp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* segmentCompare(ctx, slot, hausdorff 0 | 1, sx, sy, sz) -> { countA, countB, countAnd, d2Ab, d2Ba, argmaxAb, argmaxBa }
 * (vx_segment_compare) */
static napi_value n_segment_compare(napi_env env, napi_callback_info info) {
  CTX_ARGS(6);
  uint32_t slot;
  int32_t hausdorff;
  double v[3];
  if (napi_get_value_uint32(env, a[1], &slot) != napi_ok || napi_get_value_int32(env, a[2], &hausdorff) != napi_ok ||
      napi_get_value_double(env, a[3], &v[0]) != napi_ok || napi_get_value_double(env, a[4], &v[1]) != napi_ok ||
      napi_get_value_double(env, a[5], &v[2]) != napi_ok)
    return throw_msg(env, "segmentCompare: slot, hausdorff and the spacing must be numbers");
  VxCompareParams cp = {slot, hausdorff, {(float)v[0], (float)v[1], (float)v[2]}};
  VxCompareResult r;
  if (vx_segment_compare(c, &cp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"countA", (double)r.count_a}, {"countB", (double)r.count_b}, {"countAnd", (double)r.count_and},
                   {"d2Ab", r.d2_ab}, {"d2Ba", r.d2_ba}};
  napi_value o = num_object(env, "segmentCompare", f, COUNT(f));
  if (o && (!set_u3(env, o, "argmaxAb", r.argmax_ab) || !set_u3(env, o, "argmaxBa", r.argmax_ba)))
    return throw_result(env, "segmentCompare");
  return o;
}

/* segmentsLabelmap(ctx, Uint32Array of slots, Uint8Array of X*Y*Z labels) -> the number of overlapping voxels
 * (vx_segments_labelmap) */
static napi_value n_segments_labelmap(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  void *slots, *labels;
  size_t n, nvox;
  uint64_t overlaps = 0;
  napi_value v;
  if (!typed_required(env, a[1], napi_uint32_array, "segmentsLabelmap: slots must be a Uint32Array", &slots, &n)) return NULL;
  if (!typed_required(env, a[2], napi_uint8_array, "segmentsLabelmap: labels must be a Uint8Array", &labels, &nvox)) return NULL;
  if (n > 0xffffffffu) return throw_msg(env, "segmentsLabelmap: too many slots");
  if (vx_segments_labelmap(c, (const uint32_t*)slots, (uint32_t)n, (uint8_t*)labels, (uint64_t)nvox, &overlaps) != VX_OK)
    return throw_msg(env, vx_last_error(c));
  NAPI_OK(napi_create_double(env, (double)overlaps, &v));
  return v;
}

static napi_value init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; } fns[] = {
      {"storeSegment", n_store_segment}, {"loadSegment", n_load_segment}, {"dropSegment", n_drop_segment},
      {"storedSegments", n_stored_segments}, {"segmentCombine", n_segment_combine}, {"segmentCompare", n_segment_compare},
      {"segmentsLabelmap", n_segments_labelmap}};
  for (size_t i = 0; i < COUNT(fns); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
        napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
      napi_throw_error(env, NULL, "volxel_napi_segments: export failed");
      return NULL;
    }
  }
  return exports;
}

NAPI_MODULE(volxel_napi_segments, init)
