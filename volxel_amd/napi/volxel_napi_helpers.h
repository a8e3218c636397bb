/*
 * volxel_napi_helpers.h -- the helpers every N-API wrapper of this directory is written from (volxel_napi.c, and
 * volxel_napi_distance.c and volxel_napi_segments.c, the addons of the distance calls and of the segment store): arguments in,
 * results out.  A context handle made by
 * volxel_napi.node is read by any of them: it is an external around a Handle.
 */
#ifndef VOLXEL_NAPI_HELPERS_H
#define VOLXEL_NAPI_HELPERS_H

#include <node_api.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "../../include/volxel_brick.h"
#include "../../include/volxel_hip.h"

/* a helper an addon may leave unused (the warning stays on for the addon's own functions) */
#if defined(__GNUC__)
#define VXN_HELPER static __attribute__((unused))
#else
#define VXN_HELPER static
#endif

#define COUNT(x) (sizeof(x) / sizeof((x)[0]))

#define NAPI_OK(call)                                                    \
  do {                                                                   \
    if ((call) != napi_ok) {                                             \
      napi_throw_error(env, NULL, "volxel_napi: N-API call failed: " #call); \
      return NULL;                                                       \
    }                                                                    \
  } while (0)

VXN_HELPER napi_value throw_msg(napi_env env, const char* msg) {
  napi_throw_error(env, NULL, msg && *msg ? msg : "volxel_hip: unknown error");
  return NULL;
}

/* the answer of a call that returns nothing: undefined, or the context's error thrown */
VXN_HELPER napi_value status(napi_env env, VxContext* c, int rc) {
  return rc == VX_OK ? NULL : throw_msg(env, vx_last_error(c));
}

/* ---- arguments in --------------------------------------------------------------------------------------------------- */
VXN_HELPER int get_args(napi_env env, napi_callback_info info, size_t n, napi_value* argv) {
  size_t argc = n;
  if (napi_get_cb_info(env, info, &argc, argv, NULL, NULL) != napi_ok || argc < n) {
    napi_throw_type_error(env, NULL, "volxel_napi: wrong number of arguments");
    return 0;
  }
  return 1;
}

/* The JS handle wraps a small box, not the context itself: destroy() empties the box, so a call made after
 * dispose() (or a second destroy) finds NULL and throws instead of touching freed memory. */
typedef struct Handle {
  VxContext* ctx;
} Handle;

VXN_HELPER Handle* get_handle(napi_env env, napi_value v) {
  void* p = NULL;
  if (napi_get_value_external(env, v, &p) != napi_ok || !p) {
    napi_throw_type_error(env, NULL, "volxel_napi: expected a context handle");
    return NULL;
  }
  return (Handle*)p;
}

VXN_HELPER VxContext* get_ctx(napi_env env, napi_value v) {
  Handle* h = get_handle(env, v);
  if (!h) return NULL;
  if (!h->ctx) {
    napi_throw_error(env, NULL, "volxel_napi: the context has been destroyed");
    return NULL;
  }
  return h->ctx;
}

/* the opening of every wrapper that takes a context: declares a[n], the arguments, and c, the live context behind a[0];
 * returns after the throw when there are fewer than n or a[0] is no live context */
#define CTX_ARGS(n)                                                   \
  napi_value a[n];                                                    \
  VxContext* c = get_args(env, info, n, a) ? get_ctx(env, a[0]) : NULL; \
  if (!c) return NULL

/* number of elements of [x, y, z] multiplied out, saturating */
VXN_HELPER uint64_t prod3(const uint32_t v[3]) { return (uint64_t)v[0] * v[1] * v[2]; }

VXN_HELPER int nullish(napi_env env, napi_value v) {
  napi_valuetype t;
  return napi_typeof(env, v, &t) == napi_ok && (t == napi_undefined || t == napi_null);
}

/* typed array -> pointer + element count (+ checks the element type) */
VXN_HELPER int typed(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len) {
  napi_typedarray_type t;
  napi_value ab;
  size_t off;
  if (napi_get_typedarray_info(env, v, &t, len, data, &ab, &off) != napi_ok || t != want) {
    napi_throw_type_error(env, NULL, "volxel_napi: typed array of the wrong element type");
    return 0;
  }
  return 1;
}

/* optional typed array argument: undefined / null -> *data = NULL */
VXN_HELPER int typed_or_null(napi_env env, napi_value v, napi_typedarray_type want, void** data, size_t* len) {
  *data = NULL;
  *len = 0;
  return nullish(env, v) ? 1 : typed(env, v, want, data, len);
}

/* mandatory typed array argument whose absence has a message of the caller's: undefined / null throw `missing` */
VXN_HELPER int typed_required(napi_env env, napi_value v, napi_typedarray_type want, const char* missing, void** data, size_t* len) {
  if (!typed_or_null(env, v, want, data, len)) return 0;
  if (!*data) throw_msg(env, missing);
  return *data != NULL;
}

VXN_HELPER int u32x3(napi_env env, napi_value arr, uint32_t out[3]) {
  for (uint32_t i = 0; i < 3; ++i) {
    napi_value e;
    if (napi_get_element(env, arr, i, &e) != napi_ok || napi_get_value_uint32(env, e, &out[i]) != napi_ok) {
      napi_throw_type_error(env, NULL, "volxel_napi: expected [x, y, z]");
      return 0;
    }
  }
  return 1;
}

VXN_HELPER napi_value prop(napi_env env, napi_value obj, const char* name) {
  napi_value v = NULL;
  napi_get_named_property(env, obj, name, &v);
  return v;
}

/* an ArrayBuffer holding exactly one `type` (of `size` bytes) -> *dst; `who` opens the message, as each caller always has */
VXN_HELPER int struct_arg(napi_env env, napi_value v, void* dst, size_t size, const char* who, const char* type) {
  void* d;
  size_t n;
  char msg[96];
  if (napi_get_arraybuffer_info(env, v, &d, &n) != napi_ok) {
    throw_msg(env, "volxel_napi: N-API call failed: napi_get_arraybuffer_info(env, a[1], &d, &n)");
    return 0;
  }
  if (n != size) {
    snprintf(msg, sizeof msg, "%s: buffer is not sizeof(%s)", who, type);
    throw_msg(env, msg);
    return 0;
  }
  memcpy(dst, d, size);
  return 1;
}

/* ---- results out ---------------------------------------------------------------------------------------------------- */
/* set_*: o[name] = the value; o, or NULL when a step failed (nothing is thrown: the caller names itself) */
VXN_HELPER napi_value set_num(napi_env env, napi_value o, const char* name, double x) {
  napi_value v;
  if (napi_create_double(env, x, &v) != napi_ok || napi_set_named_property(env, o, name, v) != napi_ok) return NULL;
  return o;
}
/* [x, y, z] of uint32, or of int32 where as_int (the mesher's cells, -1 included) */
VXN_HELPER napi_value set_x3(napi_env env, napi_value o, const char* name, const uint32_t* x, int as_int) {
  napi_value arr, v;
  if (napi_create_array_with_length(env, 3, &arr) != napi_ok) return NULL;
  for (uint32_t i = 0; i < 3; ++i)
    if ((as_int ? napi_create_int32(env, (int32_t)x[i], &v) : napi_create_uint32(env, x[i], &v)) != napi_ok ||
        napi_set_element(env, arr, i, v) != napi_ok)
      return NULL;
  if (napi_set_named_property(env, o, name, arr) != napi_ok) return NULL;
  return o;
}
VXN_HELPER napi_value set_u3(napi_env env, napi_value o, const char* name, const uint32_t* x) { return set_x3(env, o, name, x, 0); }
VXN_HELPER napi_value set_bool(napi_env env, napi_value o, const char* name, int x) {
  napi_value v;
  if (napi_get_boolean(env, x != 0, &v) != napi_ok || napi_set_named_property(env, o, name, v) != napi_ok) return NULL;
  return o;
}

VXN_HELPER napi_value throw_result(napi_env env, const char* who) {
  char msg[96];
  snprintf(msg, sizeof msg, "%s: could not build the result", who);
  return throw_msg(env, msg);
}

/* names + doubles: what every *Stats call and getCounters return (u64 counts travel as doubles, exact up to 2^53) */
typedef struct Num {
  const char* name;
  double value;
} Num;

VXN_HELPER napi_value set_nums(napi_env env, napi_value o, const Num* f, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (!set_num(env, o, f[i].name, f[i].value)) return NULL;
  return o;
}

VXN_HELPER napi_value num_object(napi_env env, const char* who, const Num* f, size_t n) {
  napi_value o;
  if (napi_create_object(env, &o) != napi_ok || !set_nums(env, o, f, n)) return throw_result(env, who);
  return o;
}

/* { count, bboxLo, bboxHi, dMin, dMax, dSum, rounds, brickVisits, converged }: what segment and every call that changes
 * the mask return */
VXN_HELPER napi_value segment_result(napi_env env, const VxSegmentResult* r) {
  const Num tail[] = {{"dMin", r->d_min}, {"dMax", r->d_max}, {"dSum", r->d_sum}, {"rounds", r->rounds},
                      {"brickVisits", (double)r->brick_visits}};
  napi_value o;
  if (napi_create_object(env, &o) != napi_ok || !set_num(env, o, "count", (double)r->count) ||
      !set_u3(env, o, "bboxLo", r->bbox_lo) || !set_u3(env, o, "bboxHi", r->bbox_hi) || !set_nums(env, o, tail, COUNT(tail)) ||
      !set_bool(env, o, "converged", r->converged))
    return throw_result(env, "segment");
  return o;
}

#endif
