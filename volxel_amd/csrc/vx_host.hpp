// vx_host.hpp -- host-only helpers of vx_api.hip: the error macros and the three owners of device resources (a device
// buffer, the carve of one allocation into typed arrays, a stage timer), and the proof of the image blocks that cannot hit the
// clip box (classify_miss_blocks).  No device code.
//
// The owners release with hipFree / hipEventDestroy, which act on the calling thread's current device.  They are only ever
// released from inside an entry point that made the context's device current first: VxContext::Volume is reset by free_volume
// (vx_upload_volume behind its VX_DEV, vx_destroy behind its hipSetDevice), everything else by the `delete` at the end of
// vx_destroy, which sets the device of each context -- each member of a device group included -- before anything is released.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/volxel_hip.h"

// what the owners need of a context (VxContext derives from it)
struct VxCore {
  int device = 0;
  hipStream_t stream = nullptr;
  std::string err;
};

#define VX_FAIL(ctx, code, ...)                       \
  do {                                                \
    char buf_[512];                                   \
    snprintf(buf_, sizeof buf_, __VA_ARGS__);         \
    (ctx)->err = buf_;                                \
    return (code);                                    \
  } while (0)

#define VX_HIP(ctx, expr)                                                                   \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess) VX_FAIL(ctx, VX_ERR_DEVICE, "%s: %s", #expr, hipGetErrorString(e_)); \
  } while (0)

namespace vx {

// A device buffer that owns its memory; cap counts elements (bytes for DevBuf<void>).  Reads as its pointer.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(DevBuf&& o) noexcept : p(std::exchange(o.p, nullptr)), cap(std::exchange(o.cap, 0)) {}
  DevBuf& operator=(DevBuf&& o) noexcept {
    if (this != &o) {
      reset();
      p = std::exchange(o.p, nullptr);
      cap = std::exchange(o.cap, 0);
    }
    return *this;
  }
  ~DevBuf() { reset(); }
  operator T*() const { return p; }
  void reset() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  // exactly n elements, whatever was there: freed first, null / 0 when the allocation fails
  int alloc(VxCore* c, size_t n) {
    reset();
    VX_HIP(c, hipMalloc(reinterpret_cast<void**>(&p), n * sizeof(std::conditional_t<std::is_void_v<T>, char, T>)));
    cap = n;
    return VX_OK;
  }
  // at least n elements: grows, never shrinks
  int ensure(VxCore* c, size_t n) { return n > cap ? alloc(c, n) : VX_OK; }
};

// One allocation carved into typed arrays.  `layout` is called twice with a Carve and takes its arrays in order, take<T>(n):
// the first pass (no base) only adds up the bytes, the second hands out the pointers, so the size and the carve cannot disagree.
struct Carve {
  uintptr_t base = 0;
  size_t off = 0;
  template <class T>
  T* take(size_t n = 1) {
    T* r = base ? reinterpret_cast<T*>(base + off) : nullptr;   // (null while measuring: what a failed allocation leaves)
    off += n * sizeof(T);
    return r;
  }
};
template <class F>
int carve(VxCore* c, DevBuf<void>& buf, F&& layout) {
  Carve measure;
  layout(measure);
  if (int rc = buf.alloc(c, measure.off)) return rc;
  Carve k{reinterpret_cast<uintptr_t>(buf.p)};
  layout(k);
  return VX_OK;
}

// ---- which 16x16-pixel blocks of the image no primary ray can hit the clip box from ----------------
// Plain float64, no device.  flags[by * nbx + bx] = 1: NO ray of the pixels [16 bx, 16 bx + 16) x [16 by, 16 by + 16), under
// any jitter, enters the box volume_aabb_min .. max; 0: one may.  Returns the number of blocks flagged.
// The proof: a perspective ray of pixel (px, py) with jitter (jx, jy) in [0, 1) leaves the camera through the continuous
// pixel coordinate (px - 1/2 + 2 jx, py - 1/2 + 2 jy) (setup_world_ray: tex + (2 j - 1) / res), at most one pixel from the
// pixel's centre.  With every corner of the box in front of the camera, a ray meets the box only if that coordinate lies in
// the convex hull of the eight projected corners.  A block is flagged when one axis -- x, y or the normal of a hull edge --
// separates the rectangle of its pixel centres from the hull by 2 pixels: the jitter's reach and one pixel of safety (fp32
// rounding of the device's ray is below 2^-10 pixel at the largest image).  The projection is derived from the matrices
// the rays use, camera_view_inv and camera_proj_inv, not from their forward forms.
// Nothing is flagged (every block may hit) for an orthographic camera, matrices that are not finite, not affine (view) or not
// a pinhole (projection), a degenerate or non-finite box, the camera inside the box, or a corner behind or within a margin
// of the camera plane.  An optimisation only: a block wrongly left unflagged costs time, never correctness.
inline uint32_t classify_miss_blocks(const VxParams& p, uint32_t W, uint32_t H, std::vector<uint8_t>& flags) {
  const uint32_t nbx = (W + 15u) / 16u, nby = (H + 15u) / 16u;
  flags.assign((size_t)nbx * nby, 0);
  if (p.camera_ortho || W == 0 || H == 0) return 0;
  const float* vi = p.camera_view_inv;
  const float* pi = p.camera_proj_inv;
  for (int i = 0; i < 16; ++i)
    if (!std::isfinite(vi[i]) || !std::isfinite(pi[i])) return 0;
  for (int i = 0; i < 3; ++i)
    if (!std::isfinite(p.volume_aabb_min[i]) || !std::isfinite(p.volume_aabb_max[i]) || !(p.volume_aabb_min[i] <= p.volume_aabb_max[i]))
      return 0;
  // view: world = R v + cam (column-major; the last row must be 0 0 0 1)
  if (vi[3] != 0.0f || vi[7] != 0.0f || vi[11] != 0.0f || vi[15] != 1.0f) return 0;
  // projection: proj_inv (nx, ny, 0, 1) = nx c0 + ny c1 + c3; a pinhole has a w that does not depend on the pixel
  if (pi[3] != 0.0f || pi[7] != 0.0f || pi[15] == 0.0f) return 0;
  const double s = pi[15] > 0.0f ? 1.0 : -1.0;   // the division by w keeps or flips the direction
  // world direction of ndc (nx, ny): proportional to s B (nx, ny, 1), B = R [c0 c1 c3]
  double B[3][3];
  for (int r = 0; r < 3; ++r) {
    const int cols[3] = {0, 4, 12};
    for (int k = 0; k < 3; ++k)
      B[r][k] = (double)vi[r] * pi[cols[k]] + (double)vi[4 + r] * pi[cols[k] + 1] + (double)vi[8 + r] * pi[cols[k] + 2];
  }
  const double c00 = B[1][1] * B[2][2] - B[1][2] * B[2][1], c01 = B[1][2] * B[2][0] - B[1][0] * B[2][2],
               c02 = B[1][0] * B[2][1] - B[1][1] * B[2][0];
  const double det = B[0][0] * c00 + B[0][1] * c01 + B[0][2] * c02;
  double scale = 0.0;
  for (auto& row : B)
    for (double x : row) scale = std::max(scale, std::fabs(x));
  if (!std::isfinite(det) || !(std::fabs(det) > 1e-12 * scale * scale * scale)) return 0;
  const double Bi[3][3] = {
      {c00 / det, (B[0][2] * B[2][1] - B[0][1] * B[2][2]) / det, (B[0][1] * B[1][2] - B[0][2] * B[1][1]) / det},
      {c01 / det, (B[0][0] * B[2][2] - B[0][2] * B[2][0]) / det, (B[0][2] * B[1][0] - B[0][0] * B[1][2]) / det},
      {c02 / det, (B[0][1] * B[2][0] - B[0][0] * B[2][1]) / det, (B[0][0] * B[1][1] - B[0][1] * B[1][0]) / det}};
  const double cam[3] = {vi[12], vi[13], vi[14]};
  bool inside = true;
  double diag2 = 0.0;
  for (int i = 0; i < 3; ++i) {
    inside = inside && cam[i] >= p.volume_aabb_min[i] && cam[i] <= p.volume_aabb_max[i];
    const double e = (double)p.volume_aabb_max[i] - p.volume_aabb_min[i];
    diag2 += e * e;
  }
  if (inside) return 0;
  // the corners in continuous pixel coordinates; depth along the central ray in world units
  const double axis_len = std::sqrt(B[0][2] * B[0][2] + B[1][2] * B[1][2] + B[2][2] * B[2][2]);
  const double margin = 1e-4 * std::sqrt(diag2) + 1e-9;
  double pt[8][2];
  for (int corner = 0; corner < 8; ++corner) {
    double d[3], h[3];
    for (int i = 0; i < 3; ++i) d[i] = (double)((corner >> i) & 1 ? p.volume_aabb_max[i] : p.volume_aabb_min[i]) - cam[i];
    for (int i = 0; i < 3; ++i) h[i] = s * (Bi[i][0] * d[0] + Bi[i][1] * d[1] + Bi[i][2] * d[2]);
    if (!(h[2] * axis_len > margin)) return 0;   // behind or near the camera plane (or NaN)
    pt[corner][0] = (h[0] / h[2] + 1.0) * 0.5 * (double)W;
    pt[corner][1] = (h[1] / h[2] + 1.0) * 0.5 * (double)H;
    if (!std::isfinite(pt[corner][0]) || !std::isfinite(pt[corner][1])) return 0;
  }
  // convex hull (monotone chain); collinear points are dropped
  int idx[8] = {0, 1, 2, 3, 4, 5, 6, 7};
  std::sort(idx, idx + 8, [&](int a, int b) { return pt[a][0] < pt[b][0] || (pt[a][0] == pt[b][0] && pt[a][1] < pt[b][1]); });
  auto cross = [&](int o, int a, int b) {
    return (pt[a][0] - pt[o][0]) * (pt[b][1] - pt[o][1]) - (pt[a][1] - pt[o][1]) * (pt[b][0] - pt[o][0]);
  };
  int hull[16], nh = 0;
  for (int i = 0; i < 8; ++i) {
    while (nh >= 2 && cross(hull[nh - 2], hull[nh - 1], idx[i]) <= 0.0) --nh;
    hull[nh++] = idx[i];
  }
  for (int i = 6, lower = nh + 1; i >= 0; --i) {
    while (nh >= lower && cross(hull[nh - 2], hull[nh - 1], idx[i]) <= 0.0) --nh;
    hull[nh++] = idx[i];
  }
  --nh;   // the last point repeats the first
  // the separating axes: x, y and the unit normal of every hull edge, each with the hull's extent along it
  struct Axis { double nx, ny, lo, hi; };
  Axis axes[10];
  int na = 0;
  axes[na++] = Axis{1.0, 0.0, 0.0, 0.0};
  axes[na++] = Axis{0.0, 1.0, 0.0, 0.0};
  for (int i = 0; i < nh && nh >= 2; ++i) {
    const int a = hull[i], b = hull[(i + 1) % nh];
    const double ex = pt[b][0] - pt[a][0], ey = pt[b][1] - pt[a][1], len = std::sqrt(ex * ex + ey * ey);
    if (len > 0.0) axes[na++] = Axis{-ey / len, ex / len, 0.0, 0.0};
  }
  for (int k = 0; k < na; ++k) {
    double lo = 1e300, hi = -1e300;
    for (int i = 0; i < 8; ++i) {
      const double t = axes[k].nx * pt[i][0] + axes[k].ny * pt[i][1];
      lo = std::min(lo, t);
      hi = std::max(hi, t);
    }
    axes[k].lo = lo;
    axes[k].hi = hi;
  }
  constexpr double GAP = 2.0;   // pixels: the jitter's reach plus one of safety
  uint32_t n = 0;
  for (uint32_t by = 0; by < nby; ++by)
    for (uint32_t bx = 0; bx < nbx; ++bx) {
      // pixel centres of the block (a ragged edge block is taken whole)
      const double x0 = 16.0 * bx + 0.5, x1 = 16.0 * bx + 15.5, y0 = 16.0 * by + 0.5, y1 = 16.0 * by + 15.5;
      bool separated = false;
      for (int k = 0; k < na && !separated; ++k) {
        const double ax = axes[k].nx, ay = axes[k].ny;
        const double rlo = std::min(ax * x0, ax * x1) + std::min(ay * y0, ay * y1);
        const double rhi = std::max(ax * x0, ax * x1) + std::max(ay * y0, ay * y1);
        separated = rlo - axes[k].hi >= GAP || axes[k].lo - rhi >= GAP;
      }
      if (separated) {
        flags[(size_t)by * nbx + bx] = 1;
        ++n;
      }
    }
  return n;
}

// The timer of N stages of a call: N + 1 events, created by the first mark.  mark(c, i) records event i on the context's
// stream; read(c) fills ms[k] with the time from event k to event k + 1 (every event recorded and complete).
template <int N>
struct StageTimer {
  hipEvent_t ev[N + 1] = {};
  double ms[N] = {};   // what the last read found
  StageTimer() = default;
  StageTimer(const StageTimer&) = delete;
  StageTimer& operator=(const StageTimer&) = delete;
  ~StageTimer() {
    for (hipEvent_t e : ev)
      if (e) (void)hipEventDestroy(e);
  }
  int mark(VxCore* c, int i) {
    for (hipEvent_t& e : ev)
      if (!e) VX_HIP(c, hipEventCreate(&e));
    VX_HIP(c, hipEventRecord(ev[i], c->stream));
    return VX_OK;
  }
  int read(VxCore* c) {
    for (int k = 0; k < N; ++k) {
      float f = 0.0f;
      VX_HIP(c, hipEventElapsedTime(&f, ev[k], ev[k + 1]));
      ms[k] = f;
    }
    return VX_OK;
  }
};

}  // namespace vx
