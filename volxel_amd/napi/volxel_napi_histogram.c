/*
 * volxel_napi_histogram.c -- the N-API addon of the histograms (vx_histogram, vx_histogram_stats; include/volxel_hip.h
 * "histograms"): volxel_napi_histogram.node, beside volxel_napi.node, volxel_napi_distance.node and volxel_napi_segments.node
 * and written from the same helpers (volxel_napi_helpers.h).  An addon of its own so that the export lists of the other three
 * stay what they were.  Every function but sizeofHistogramParams takes a context handle made by volxel_napi.node's create.
 */
#include "volxel_napi_helpers.h"

/* sizeofHistogramParams() -> sizeof(VxHistogramParams): what viewer.js checks its parse of the header against */
static napi_value n_sizeof_histogram_params(napi_env env, napi_callback_info info) {
  napi_value v;
  (void)info;
  NAPI_OK(napi_create_uint32(env, (uint32_t)sizeof(VxHistogramParams), &v));
  return v;
}

/* histogram(ctx, ArrayBuffer holding a VxHistogramParams, Float64Array of one element per bin) -> { count, below, above, dSum,
 * dSum2, dMin, dMax }; the bins are written into the array as doubles (every count is below 2^53) (vx_histogram) */
static napi_value n_histogram(napi_env env, napi_callback_info info) {
  CTX_ARGS(3);
  VxHistogramParams hp;
  void* dst;
  size_t n;
  if (!struct_arg(env, a[1], &hp, sizeof hp, "histogram", "VxHistogramParams")) return NULL;
  if (!typed_required(env, a[2], napi_float64_array, "histogram: counts must be a Float64Array", &dst, &n)) return NULL;
  if (n < 1 || n > VX_HIST_MAX_BINS) return throw_msg(env, "histogram: counts must hold 1 .. 4096 bins");
  uint64_t* counts = (uint64_t*)malloc(n * sizeof *counts);
  if (!counts) return throw_msg(env, "histogram: out of memory");
  VxHistogramResult r;
  if (vx_histogram(c, &hp, counts, (uint32_t)n, &r) != VX_OK) {
    free(counts);
    return throw_msg(env, vx_last_error(c));
  }
  for (size_t i = 0; i < n; ++i) ((double*)dst)[i] = (double)counts[i];
  free(counts);
  const Num f[] = {{"count", (double)r.count}, {"below", (double)r.below}, {"above", (double)r.above}, {"dSum", r.d_sum},
                   {"dSum2", r.d_sum2}, {"dMin", r.d_min}, {"dMax", r.d_max}};
  return num_object(env, "histogram", f, COUNT(f));
}

/* histogramStats(ctx) -> { launches, histogramMs, momentsMs } (vx_histogram_stats) */
static napi_value n_histogram_stats(napi_env env, napi_callback_info info) {
  CTX_ARGS(1);
  uint32_t launches = 0;
  double ms[2] = {0.0, 0.0};
  if (vx_histogram_stats(c, &launches, ms) != VX_OK) return throw_msg(env, vx_last_error(c));
  const Num f[] = {{"launches", launches}, {"histogramMs", ms[0]}, {"momentsMs", ms[1]}};
  return num_object(env, "histogramStats", f, COUNT(f));
}

static napi_value init(napi_env env, napi_value exports) {
  static const struct { const char* name; napi_callback fn; } fns[] = {
      {"sizeofHistogramParams", n_sizeof_histogram_params}, {"histogram", n_histogram}, {"histogramStats", n_histogram_stats}};
  for (size_t i = 0; i < COUNT(fns); ++i) {
    napi_value f;
    if (napi_create_function(env, fns[i].name, NAPI_AUTO_LENGTH, fns[i].fn, NULL, &f) != napi_ok ||
        napi_set_named_property(env, exports, fns[i].name, f) != napi_ok) {
      napi_throw_error(env, NULL, "volxel_napi_histogram: export failed");
      return NULL;
    }
  }
  return exports;
}

NAPI_MODULE(volxel_napi_histogram, init)
