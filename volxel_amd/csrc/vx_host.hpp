// vx_host.hpp -- host-only helpers of the host units (vx_api*.hip): the error macros and the three owners of device resources (a device
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
#include <cstring>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/volxel_hip.h"

// (namespace vx is hidden in the host headers: the library exports its C ABI and nothing of its own helpers)

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

namespace vx __attribute__((visibility("hidden"))) {

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

// ---- exact empty-space skipping: host-side construction of the macro-cell bitmask -------------
// Rule (restated independently by the oracle): TF bin i is dead when its alpha
// is 0 or it lies wholly outside the sample range (one-bin margin); a brick is transparent when
// every bin from I(min)-1 to I(max)+1 is dead, I(x) = floor(x*density_scale*inv_maj*L); a macro
// cell of w = 2^level bricks per axis is empty when the w+1 bricks per axis that can hold a tap of
// its cells (bricks m*w-1 .. m*w+w-1; value 0 outside the grid) are all transparent.
inline float f16_bits_to_float(uint16_t h) {
  _Float16 v;
  memcpy(&v, &h, 2);
  return (float)v;
}
inline int skip_level_for(const uint32_t extent[3]) {
  for (int g = 1; g <= 3; ++g) {
    uint64_t n = 1;
    for (int a = 0; a < 3; ++a) n *= (uint64_t)(extent[a] >> (3 + g)) + 1u;
    if (n <= 65536u) return g;
  }
  return 3;
}
inline void compute_skip_mask(const VxParams& p, const uint32_t* range_packed, const uint32_t bc[3],
                              const uint32_t extent[3], const float* tf_rgba, uint32_t L,
                              std::vector<uint32_t>& bits, int& level_out, uint32_t md[3]) {
  const float lf = (float)L;
  // prefix count of live bins -> O(1) "any live bin in [a, b]"
  std::vector<uint32_t> live(L + 1, 0);
  for (uint32_t i = 0; i < L; ++i) {
    bool dead = tf_rgba[4 * (size_t)i + 3] == 0.0f || (float)((int)i + 2) / lf < p.sample_range[0] ||
                (float)((int)i - 1) / lf > p.sample_range[1];
    live[i + 1] = live[i] + (dead ? 0u : 1u);
  }
  auto transparent = [&](float lo, float hi) {
    float fa = floorf(((lo * p.volume_density_scale) * p.volume_inv_maj) * lf);
    float fb = floorf(((hi * p.volume_density_scale) * p.volume_inv_maj) * lf);
    // v_cvt_i32_f32 semantics: NaN -> 0, saturating
    auto f2i = [](float x) -> int64_t { return x != x ? 0 : (x >= 2147483648.0f ? 2147483647ll : (x <= -2147483648.0f ? -2147483648ll : (int64_t)x)); };
    int64_t a = f2i(fa) - 1, b = f2i(fb) + 1;
    if (a < 0) a = 0;
    if (b > (int64_t)L - 1) b = (int64_t)L - 1;
    if (b < a) return true;
    return live[(size_t)b + 1] - live[(size_t)a] == 0u;
  };
  const size_t nb = (size_t)bc[0] * bc[1] * bc[2];
  std::vector<uint8_t> opaque(nb);
  for (size_t i = 0; i < nb; ++i) {
    uint32_t pk = range_packed[i];
    opaque[i] = transparent(f16_bits_to_float((uint16_t)(pk >> 16)), f16_bits_to_float((uint16_t)pk)) ? 0 : 1;
  }
  const uint8_t zero_opaque = transparent(0.0f, 0.0f) ? 0 : 1;
  const int level = skip_level_for(extent);
  level_out = level;
  const int w = 1 << level;
  for (int a = 0; a < 3; ++a) md[a] = (extent[a] >> (3 + level)) + 1u;
  // separable OR over the window [m*w-1, m*w+w-1] per axis (out-of-grid bricks count as value 0)
  std::vector<uint8_t> ax((size_t)md[0] * bc[1] * bc[2]), ay((size_t)md[0] * md[1] * bc[2]);
  for (uint32_t z = 0; z < bc[2]; ++z)
    for (uint32_t y = 0; y < bc[1]; ++y)
      for (uint32_t m = 0; m < md[0]; ++m) {
        uint8_t o = 0;
        for (int b = (int)m * w - 1; b <= (int)m * w + w - 1; ++b)
          o |= (b < 0 || (uint32_t)b >= bc[0]) ? zero_opaque : opaque[((size_t)z * bc[1] + y) * bc[0] + b];
        ax[((size_t)z * bc[1] + y) * md[0] + m] = o;
      }
  for (uint32_t z = 0; z < bc[2]; ++z)
    for (uint32_t m = 0; m < md[1]; ++m)
      for (uint32_t x = 0; x < md[0]; ++x) {
        uint8_t o = 0;
        for (int b = (int)m * w - 1; b <= (int)m * w + w - 1; ++b)
          o |= (b < 0 || (uint32_t)b >= bc[1]) ? zero_opaque : ax[((size_t)z * bc[1] + b) * md[0] + x];
        ay[((size_t)z * md[1] + m) * md[0] + x] = o;
      }
  const size_t n = (size_t)md[0] * md[1] * md[2];
  bits.assign((n + 31) / 32, 0u);
  for (uint32_t m = 0; m < md[2]; ++m)
    for (uint32_t y = 0; y < md[1]; ++y)
      for (uint32_t x = 0; x < md[0]; ++x) {
        uint8_t o = 0;
        for (int b = (int)m * w - 1; b <= (int)m * w + w - 1; ++b)
          o |= (b < 0 || (uint32_t)b >= bc[2]) ? zero_opaque : ay[((size_t)b * md[1] + y) * md[0] + x];
        if (!o) {
          size_t i = ((size_t)m * md[1] + y) * md[0] + x;
          bits[i >> 5] |= 1u << (i & 31);
        }
      }
}

// ---- range skipping of the intensity projections: host-side construction of the density bounds ----------------------
// Per macro cell of the empty-space grid above (level, dims), {lo, hi} with lo <= d <= hi for every density
// d = (density_scale * mix) * inv_maj the device can compute at a sample of the cell.  Such a sample (mask index
// floor(q) + 1 in the cell) takes its eight taps from the w + 1 bricks per axis m*w-1 .. m*w+w-1 that compute_skip_mask
// ORs (a tap outside the grid reads 0), and a tap of brick b is decoded inside b's own range [min, max] (the f16 pair).
// Rounding, argued against a relative margin of 2^-16 and an absolute one of 2^-100:
//   * a decoded voxel, fma(c/255, max - min, min), lands at most an ulp or two beyond [min, max] (relative 2^-22);
//   * a mix fma(b, t, a * (1 - t)): 1 - t and the product round once each, the fma once: with weights t, 1 - t in [0, 1] the
//     result is within 3 rounding errors (2^-24 each, of the larger operand) of a convex combination, and the trilinear is
//     three nested mixes -- at most ~10 rounding errors of max(|lo|, |hi|) in all, below 2^-20 relative;
//   * the products by density_scale and inv_maj add one rounding each, and a device that flushes a denormal moves a value by
//     less than 2^-126.
// Bounds widened by 2^-16 of the magnitude and by 2^-100 hold with a margin of more than 16x.  A density_scale or inv_maj
// that is <= 0 or not finite turns the map around or breaks it: then the bounds are {-inf, +inf} and nothing is skipped.
inline void compute_projection_bounds(const VxParams& p, const uint32_t* range_packed, const uint32_t bc[3],
                                      const uint32_t extent[3], std::vector<float>& lohi, int& level_out, uint32_t md[3]) {
  const int level = skip_level_for(extent);
  level_out = level;
  const int w = 1 << level;
  for (int a = 0; a < 3; ++a) md[a] = (extent[a] >> (3 + level)) + 1u;
  const size_t n = (size_t)md[0] * md[1] * md[2];
  lohi.assign(2 * n, 0.0f);
  const float s = p.volume_density_scale, im = p.volume_inv_maj;
  if (!(s > 0.0f) || !(im > 0.0f) || !std::isfinite(s) || !std::isfinite(im)) {
    for (size_t i = 0; i < n; ++i) { lohi[2 * i] = -INFINITY; lohi[2 * i + 1] = INFINITY; }
    return;
  }
  // per-brick ranges, then separable min / max over the window [m*w-1, m*w+w-1] per axis (out-of-grid bricks read 0)
  const size_t nb = (size_t)bc[0] * bc[1] * bc[2];
  std::vector<float> bmin(nb), bmax(nb);
  for (size_t i = 0; i < nb; ++i) {
    const uint32_t pk = range_packed[i];
    const float a = f16_bits_to_float((uint16_t)(pk >> 16)), b = f16_bits_to_float((uint16_t)pk);
    bmin[i] = std::min(a, b);
    bmax[i] = std::max(a, b);
  }
  auto reduce = [&](const std::vector<float>& src, uint32_t sx, uint32_t sy, uint32_t sz, int axis, bool hi) {
    const uint32_t dims_in[3] = {sx, sy, sz};
    uint32_t d[3] = {sx, sy, sz};
    d[axis] = md[axis];
    std::vector<float> out((size_t)d[0] * d[1] * d[2]);
    for (uint32_t z = 0; z < d[2]; ++z)
      for (uint32_t y = 0; y < d[1]; ++y)
        for (uint32_t x = 0; x < d[0]; ++x) {
          uint32_t at[3] = {x, y, z};
          const int m = (int)at[axis];
          float r = 0.0f;
          bool first = true;
          for (int b = m * w - 1; b <= m * w + w - 1; ++b) {
            float v = 0.0f;
            if (b >= 0 && (uint32_t)b < dims_in[axis]) {
              at[axis] = (uint32_t)b;
              v = src[((size_t)at[2] * dims_in[1] + at[1]) * dims_in[0] + at[0]];
            }
            r = first ? v : (hi ? std::max(r, v) : std::min(r, v));
            first = false;
          }
          out[((size_t)z * d[1] + y) * d[0] + x] = r;
        }
    return out;
  };
  for (int hi = 0; hi < 2; ++hi) {
    const std::vector<float>& b0 = hi ? bmax : bmin;
    std::vector<float> rx = reduce(b0, bc[0], bc[1], bc[2], 0, hi);
    std::vector<float> ry = reduce(rx, md[0], bc[1], bc[2], 1, hi);
    std::vector<float> rz = reduce(ry, md[0], md[1], bc[2], 2, hi);
    for (size_t i = 0; i < n; ++i) {
      const double v = rz[i];   // voxel units
      const double d = v * (double)s * (double)im;
      const double widened = hi ? d + std::fabs(d) * 0x1p-16 + 0x1p-100 : d - std::fabs(d) * 0x1p-16 - 0x1p-100;
      float f = (float)widened;   // then one more step outwards against the conversion's rounding
      f = std::nextafter(f, hi ? INFINITY : -INFINITY);
      lohi[2 * i + hi] = f;
    }
  }
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
