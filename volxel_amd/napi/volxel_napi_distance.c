/*
 * volxel_napi_distance.c -- the N-API addon of the distance calls (vx_segment_distance, vx_distance_read, vx_segment_margin,
 * vx_distance_stats; include/volxel_hip.h "distances and margins"): volxel_napi_distance.node, beside volxel_napi.node and written
 * from the same helpers (volxel_napi_helpers.h).  Every function takes a context handle made by volxel_napi.node's create.
 */
#include "volxel_napi_helpers.h"

/* segmentMargin(ctx, op 0 .. 3, radius, sx, sy, sz, band 0 | 1) -> what segment returns, for the new mask (vx_segment_margin) */
static napi_value n_segment_margin(napi_env env, napi_callback_info info) {
  CTX_ARGS(7);
  int32_t op, band;
  double v[4];
  if (napi_get_value_int32(env, a[1], &op) != napi_ok || napi_get_value_double(env, a[2], &v[0]) != napi_ok ||
      napi_get_value_double(env, a[3], &v[1]) != napi_ok || napi_get_value_double(env, a[4], &v[2]) != napi_ok ||
      napi_get_value_double(env, a[5], &v[3]) != napi_ok || napi_get_value_int32(env, a[6], &band) != napi_ok)
    return throw_msg(env, "segmentMargin: op, radius, the spacing and band must be numbers");
  VxMarginParams mp = {op, (float)v[0], {(float)v[1], (float)v[2], (float)v[3]}, band};
  VxSegmentResult r;
  if (vx_segment_margin(c, &mp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  return segment_result(env, &r);
}

/* segmentDistance(ctx, sx, sy, sz, maxDistance, side 0 | 1) -> { finite, maxD2, argmax } (vx_segment_distance) */
static napi_value n_segment_distance(napi_env env, napi_callback_info info) {
  CTX_ARGS(6);
  int32_t side;
  double v[4];
  if (napi_get_value_double(env, a[1], &v[0]) != napi_ok || napi_get_value_double(env, a[2], &v[1]) != napi_ok ||
      napi_get_value_double(env, a[3], &v[2]) != napi_ok || napi_get_value_double(env, a[4], &v[3]) != napi_ok ||
      napi_get_value_int32(env, a[5], &side) != napi_ok)
    return throw_msg(env, "segmentDistance: the spacing, maxDistance and side must be numbers");
  VxDistanceParams dp = {{(float)v[0], (float)v[1], (float)v[2]}, (float)v[3], side};
  VxDistanceResult r;
  if (vx_segment_distance(c, &dp, &r) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"finite", (double)r.finite}, {"maxD2", r.max_d2}};
  napi_value o = num_object(env, "segmentDistance", f, COUNT(f));
  if (o && !set_u3(env, o, "argmax", r.argmax)) return throw_result(env, "segmentDistance");
  return o;
}

/* distanceRead(ctx, Float32Array of X*Y*Z squared distances) (vx_distance_read) */
static napi_value n_distance_read(napi_env env, napi_callback_info info) {
  CTX_ARGS(2);
  void* out;
  size_t n;
  if (!typed_required(env, a[1], napi_float32_array, "distanceRead: d2 must be a Float32Array", &out, &n)) return NULL;
  return status(env, c, vx_distance_read(c, (float*)out, (uint64_t)n));
}

/* distanceStats(ctx) -> { launches, xMs, yMs, zMs, compareMs } (vx_distance_stats) */
static napi_value n_distance_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t launches = 0;
  double ms[4] = {0.0, 0.0, 0.0, 0.0};
  if (vx_distance_stats(c, &launches, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"launches", launches}, {"xMs", ms[0]}, {"yMs", ms[1]}, {"zMs", ms[2]}, {"compareMs", ms[3]}};
  return num_object(env, "distanceStats", f, COUNT(f));
}

static napi_value init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; } fns[] = {
      {"segmentMargin", n_segment_margin}, {"segmentDistance", n_segment_distance}, {"distanceRead", n_distance_read},
      {"distanceStats", n_distance_stats}};
  for (size_t i = 0; i < COUNT(fns); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
        napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
      napi_throw_error(env, NULL, "volxel_napi_distance: export failed");
      return NULL;
    }
  }
  return exports;
}

NAPI_MODULE(volxel_napi_distance, init)
