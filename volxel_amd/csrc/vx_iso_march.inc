// vx_iso_march.inc -- the body of the isosurface kernels (vx_iso.hpp), included INSIDE iso_first_hit<LAYOUT, SKIP> and
// iso_first_hit_seg<LAYOUT> (textual, as vx_dvr_lds_march.inc: the unmasked kernels compile to what they were before the masked
// form existed).  In scope: LAYOUT, SKIP, `constexpr bool SEGV`, the kernel arguments p, v, ip, ib, rgba_out, hit_out, counts,
// and `segm` / `seg_inv` (the segment view; unused unless SEGV).  Every tap -- march, bisection and gradient alike -- goes
// through iso_cell.
  const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63u;
  const uint32_t x = ip.window[0] + blockIdx.x * 16u + (wave & 1u) * 8u + (lane & 7u);
  const uint32_t y = ip.window[1] + blockIdx.y * 16u + (wave >> 1) * 8u + (lane >> 3);
  const bool in_window = x < ip.window[2] && y < ip.window[3];   // no lane returns early: the counts are whole-wave sums

  // DVR's ray (dvr_setup without jitter; the per-launch ray terms evaluated here: the same bits)
  const float tex_x = tex_coord((int)x, p.res[0], nullptr, 0), tex_y = tex_coord((int)y, p.res[1], nullptr, 1);
  const Ray ray = setup_world_ray(p, tex_x, tex_y, 0.5f, 0.5f);
  float near = 0.0f, far = 0.0f;
  const bool box = in_window && ray_box_intersection(ray, p.volume_aabb_min, p.volume_aabb_max, near, far);
  V3 ipos, idir;
  to_index(p, ray, ipos, idir);
  const float dt = p.dvr_step_voxels / sqrtf(dot3(idir, idir));
  const float t0 = fma_(0.5f, dt, near);
  const float xq = (far - t0) / dt;
  const float nf = (box && xq > 0.0f) ? fminf(ceilf(xq), (float)p.dvr_max_steps) : 0.0f;
  const V3 dq = v3(dt * idir.x, dt * idir.y, dt * idir.z);
  const V3 q0 = v3(fma_(t0, idir.x, ipos.x) - 0.5f, fma_(t0, idir.y, ipos.y) - 0.5f, fma_(t0, idir.z, ipos.z) - 0.5f);

  const float scale = p.volume_density_scale, inv_maj = p.volume_inv_maj, iso = ip.iso;
  auto density = [&](float s) {
    const float qx = fma_(s, dq.x, q0.x), qy = fma_(s, dq.y, q0.y), qz = fma_(s, dq.z, q0.z);
    const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
    return iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, f2i(flx), f2i(fly), f2i(flz), qx - flx, qy - fly, qz - flz) * inv_maj;
  };

  // the march: the first k < n with d_k >= iso
  float kf = 0.0f;
  uint32_t n_samples = 0, n_skipped = 0;
  bool found = false;
#pragma unroll 1
  for (; kf < nf; kf += 1.0f) {
    if (SKIP) {
      const float qx = fma_(kf, dq.x, q0.x), qy = fma_(kf, dq.y, q0.y), qz = fma_(kf, dq.z, q0.z);
      uint32_t cx = (uint32_t)(f2i(floorf(qx)) + 1), cy = (uint32_t)(f2i(floorf(qy)) + 1), cz = (uint32_t)(f2i(floorf(qz)) + 1);
      cx = cx < ib.cmax[0] ? cx : ib.cmax[0];
      cy = cy < ib.cmax[1] ? cy : ib.cmax[1];
      cz = cz < ib.cmax[2] ? cz : ib.cmax[2];
      if (ib.hi[((cz >> ib.sh) * ib.md1 + (cy >> ib.sh)) * ib.md0 + (cx >> ib.sh)] < iso) {
        n_skipped += 1u;
        continue;
      }
    }
    n_samples += 1u;
    if (density(kf) >= iso) {
      found = true;
      break;
    }
  }
  const bool cap = found && kf == 0.0f;

  // bisection on the sample parameter between the last sample below the threshold and the first at or above it
  float s = kf;
  if (found && !cap) {
    float lo = kf - 1.0f, hi = kf;
#pragma unroll 1
    for (uint32_t i = 0; i < ip.refine; ++i) {
      const float mid = 0.5f * (lo + hi);
      if (density(mid) >= iso) hi = mid;
      else lo = mid;
    }
    s = hi;
  }

  if (in_window) {
    const size_t o = (size_t)(y - ip.window[1]) * (ip.window[2] - ip.window[0]) + (x - ip.window[0]);
    float4 h = make_float4(0.0f, 0.0f, 0.0f, -1.0f), c = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (found) {
      const float t = fma_(s, dt, t0);
      h = make_float4(fma_(t, ray.d.x, ray.o.x), fma_(t, ray.d.y, ray.o.y), fma_(t, ray.d.z, ray.o.z), t);
      // Phong's gradient (Frame::dvr<PHONG>): central differences one voxel either side in the cell frame of q(s*)
      V3 g = v3(0.0f, 0.0f, 0.0f);
      if (!cap) {
        const float qx = fma_(s, dq.x, q0.x), qy = fma_(s, dq.y, q0.y), qz = fma_(s, dq.z, q0.z);
        const float flx = floorf(qx), fly = floorf(qy), flz = floorf(qz);
        const float fx = qx - flx, fy = qy - fly, fz = qz - flz;
        const int cx = f2i(flx), cy = f2i(fly), cz = f2i(flz);
        const float gx = iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx + 1, cy, cz, fx, fy, fz) - iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx - 1, cy, cz, fx, fy, fz);
        const float gy = iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx, cy + 1, cz, fx, fy, fz) - iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx, cy - 1, cz, fx, fy, fz);
        const float gz = iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx, cy, cz + 1, fx, fy, fz) - iso_cell<LAYOUT, SEGV>(v, segm, seg_inv, scale, cx, cy, cz - 1, fx, fy, fz);
        g = v3(gx * p.density_transform_inv[0], gy * p.density_transform_inv[5], gz * p.density_transform_inv[10]);
      }
      const float g2 = dot3(g, g);
      const V3 n = (!cap && g2 > 1e-12f) ? scale3(g, -rsq_fast(g2)) : v3(-ray.d.x, -ray.d.y, -ray.d.z);
      const V3 nl = v3(-p.light_dir[0], -p.light_dir[1], -p.light_dir[2]);
      const V3 hv = normalize3(sub3(nl, ray.d));
      const float diff = fma_(ip.kd, gl_max(0.0f, dot3(n, nl)), ip.ka);
      const float spec = ip.ks * pow_fast(gl_max(0.0f, dot3(n, hv)), ip.shininess);
      c = make_float4(fma_(ip.color[0], diff, spec), fma_(ip.color[1], diff, spec), fma_(ip.color[2], diff, spec), 1.0f);
    }
    if (rgba_out) rgba_out[o] = c;
    if (hit_out) hit_out[o] = h;
  }

  const uint32_t n_rays = (uint32_t)__builtin_popcountll(__ballot(box));
  const uint32_t n_hits = (uint32_t)__builtin_popcountll(__ballot(found));
  const uint32_t n_refined = (uint32_t)__builtin_popcountll(__ballot(found && !cap));
  n_samples = wave_sum(n_samples);
  n_skipped = wave_sum(n_skipped);
  if (lane == 0u) {
    if (n_rays) atomicAdd(&counts[ISO_RAYS], (unsigned long long)n_rays);
    if (n_hits) atomicAdd(&counts[ISO_HITS], (unsigned long long)n_hits);
    if (n_samples) atomicAdd(&counts[ISO_SAMPLES], (unsigned long long)n_samples);
    if (n_refined) atomicAdd(&counts[ISO_REFINE], (unsigned long long)n_refined * ip.refine);
    if (n_skipped) atomicAdd(&counts[ISO_SKIPPED], (unsigned long long)n_skipped);
  }
