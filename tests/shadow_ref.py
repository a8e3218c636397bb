"""NumPy restatement of shadowed DVR ("light grid"): the light grid toward the directional light and the
DVR image whose contributing samples add dT * T_L.  Built on oracle/np_oracle.py (NpVolume.trilinear_q, transfer), which
reproduces the device's densities bit for bit; with T_L = 1 the image is np_oracle.dvr_image's."""
import math

import numpy as np

from oracle import np_oracle as NP

F32 = np.float32
fma = NP.fma


def _gmin(a, b):   # GLSL min / max (utils.glsl slab test), as vx_device.hpp gl_min / gl_max
    return np.where(b < a, b, a)


def _gmax(a, b):
    return np.where(a < b, b, a)


def _slab(o, d, lo, hi):
    """ray_box_intersection (utils.glsl:61-69) for origins o (3 arrays) and one direction d"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = [F32(1) / F32(x) for x in d]
        a = [(F32(lo[i]) - o[i]) * inv[i] for i in range(3)]
        b = [(F32(hi[i]) - o[i]) * inv[i] for i in range(3)]
    tmin = [_gmin(x, y) for x, y in zip(a, b)]
    tmax = [_gmax(x, y) for x, y in zip(a, b)]
    near = _gmax(np.zeros_like(tmin[0]), _gmax(tmin[0], _gmax(tmin[1], tmin[2])))
    far = _gmin(tmax[0], _gmin(tmax[1], tmax[2]))
    return near <= far, near, far


def light_march(p, extent, stride):
    """what vx_api.hip light_march computes on the host: idir, dt, the clip box in index space, nodes per axis"""
    m = np.asarray(p.density_transform_inv[:], dtype=F32)
    ld = [-F32(p.light_dir[i]) for i in range(3)]
    idir = [fma(m[8 + i], ld[2], fma(m[4 + i], ld[1], m[i] * ld[0])) for i in range(3)]
    dt = F32(p.dvr_step_voxels) / np.sqrt(fma(idir[2], idir[2], fma(idir[1], idir[1], idir[0] * idir[0])))
    lo, hi = [np.inf] * 3, [-np.inf] * 3
    for corner in range(8):
        w = [F32(p.volume_aabb_max[i] if (corner >> i) & 1 else p.volume_aabb_min[i]) for i in range(3)]
        for i in range(3):
            q = fma(m[12 + i], F32(1), fma(m[8 + i], w[2], fma(m[4 + i], w[1], m[i] * w[0])))
            lo[i], hi[i] = min(lo[i], q), max(hi[i], q)
    n = [(int(extent[i]) - 1 + stride - 1) // stride + 1 for i in range(3)]
    return [F32(x) for x in idir], F32(dt), [F32(x) for x in lo], [F32(x) for x in hi], n


def inside_nodes(lo, hi, n, stride):
    """per axis the first and last node whose position stride * i + 1/2 lies inside the clip box [lo, hi]"""
    ilo, ihi = [], []
    for a in range(3):
        l = min(max(math.ceil((float(lo[a]) - 0.5) / stride), 0), n[a] - 1)
        h = min(max(math.floor((float(hi[a]) - 0.5) / stride), l), n[a] - 1)
        ilo.append(l)
        ihi.append(h)
    return ilo, ihi


def light_grid(p, grid, tf, L, stride):
    """(T, samples): T[k, j, i] = exp(-tau) of the light march from node (i, j, k), and the samples all marches took"""
    idir, dt, lo, hi, n = light_march(p, grid.index_extent, stride)
    k, j, i = np.meshgrid(np.arange(n[2]), np.arange(n[1]), np.arange(n[0]), indexing="ij")
    o = [(F32(stride) * a.astype(F32) + F32(0.5)).astype(F32) for a in (i, j, k)]
    hit, near, far = _slab(o, idir, lo, hi)
    with np.errstate(divide="ignore", invalid="ignore"):   # nodes whose march misses the box: inf / NaN, never sampled
        t0 = fma(F32(0.5), dt, near)
        x = (far - t0) / dt
        q0 = [fma(t0, idir[a], o[a]) - F32(0.5) for a in range(3)]
    ns = np.where(hit & (x > 0), np.minimum(np.ceil(x), F32(p.dvr_max_steps)), F32(0)).astype(F32)
    dq = [dt * idir[a] for a in range(3)]
    vol = NP.NpVolume(grid)
    tau = np.zeros(ns.shape, dtype=F32)
    done = np.zeros(ns.shape, dtype=bool)
    ert = F32(p.dvr_ert_tau)
    samples, m = 0, 0
    while True:
        alive = (F32(m) < ns) & ~done
        if not alive.any():
            break
        idx = np.nonzero(alive)
        samples += len(idx[0])
        q = [fma(F32(m), dq[a][idx] if np.ndim(dq[a]) else dq[a], q0[a][idx]) for a in range(3)]
        d = vol.trilinear_q(p.volume_density_scale, *q)
        a = NP.transfer(tf, L, p.sample_range, d * F32(p.volume_inv_maj))[..., 3]
        t = fma(a * F32(p.volume_maj), dt, tau[idx])
        tau[idx] = t
        if ert > 0:
            done[idx] = t >= ert
        m += 1
    return np.exp(-tau.astype(np.float64)).astype(F32), samples


def shadow_lookup(T, stride, qx, qy, qz, ilo, ihi):
    """T_L at cell-frame positions q: the trilinear of the light grid at q / s, clamped per axis to the nodes inside the clip
    box [ilo, ihi] (inside_nodes)"""
    n = T.shape[::-1]
    inv = F32(1) / F32(stride)
    ii, ff = [], []
    for q, na, l, h in zip((qx, qy, qz), n, ilo, ihi):
        g = np.fmin(np.fmax(np.asarray(q, dtype=F32) * inv, F32(l)), F32(h))
        c = np.minimum(np.floor(g), F32(na - 2))
        ii.append(c.astype(np.int64))
        ff.append((g - c).astype(F32))
    x, y, z = ii

    def mix(a, b, t):
        return fma(b, t, a * (F32(1) - t))
    lx0 = mix(T[z, y, x], T[z, y, x + 1], ff[0])
    lx1 = mix(T[z, y + 1, x], T[z, y + 1, x + 1], ff[0])
    hx0 = mix(T[z + 1, y, x], T[z + 1, y, x + 1], ff[0])
    hx1 = mix(T[z + 1, y + 1, x], T[z + 1, y + 1, x + 1], ff[0])
    return mix(mix(lx0, lx1, ff[1]), mix(hx0, hx1, ff[1]), ff[2])


def dvr_image_shadowed(p, grid, tf, L, T=None, stride=1, max_iter=100000):
    """np_oracle.dvr_image with the shadow term: a contributing sample adds w = dT * T_L(q).  T=None: T_L = 1 (plain DVR).
    Returns (image, samples, tf_samples)."""
    W, H = p.res[0], p.res[1]
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    tex_x = (px.astype(F32) + F32(0.5)) / F32(W)
    tex_y = (py.astype(F32) + F32(0.5)) / F32(H)
    one, zero = np.ones_like(tex_x), np.zeros_like(tex_x)
    mm = NP._mat_mul
    cw = mm(p.camera_view_inv[:], zero, zero, zero, one)
    cam = [cw[i] / cw[3] for i in range(3)]
    vp = mm(p.camera_proj_inv[:], fma(tex_x, F32(2), F32(-1)), fma(tex_y, F32(2), F32(-1)), zero, one)
    vv = [vp[i] / vp[3] for i in range(3)]
    wp = mm(p.camera_view_inv[:], vv[0], vv[1], vv[2], one)
    d = [wp[i] / wp[3] - cam[i] for i in range(3)]
    if getattr(p, "camera_ortho", 0):
        npt = mm(p.camera_proj_inv[:], fma(tex_x, F32(2), F32(-1)), fma(tex_y, F32(2), F32(-1)), -one, one)
        wo = mm(p.camera_view_inv[:], npt[0] / npt[3], npt[1] / npt[3], npt[2] / npt[3], one)
        cam = [wo[i] / wo[3] for i in range(3)]
        wd = mm(p.camera_view_inv[:], zero, zero, -one, zero)
        d = [wd[i] for i in range(3)]
    dd = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))
    inv = F32(1) / np.sqrt(dd)
    d = [a * inv for a in d]
    hit, near, far = _slab(cam, d, p.volume_aabb_min, p.volume_aabb_max)
    if T is not None:
        _, _, blo, bhi, nn = light_march(p, grid.index_extent, stride)
        ilo, ihi = inside_nodes(blo, bhi, nn, stride)
    ip = mm(p.density_transform_inv[:], cam[0], cam[1], cam[2], one)
    idr = mm(p.density_transform_inv[:], d[0], d[1], d[2], zero)
    il = fma(idr[2], idr[2], fma(idr[1], idr[1], idr[0] * idr[0]))
    dt = F32(p.dvr_step_voxels) / np.sqrt(il)
    t0 = fma(F32(0.5), dt, near)
    vol = NP.NpVolume(grid)
    C = [np.zeros_like(tex_x) for _ in range(3)]
    Tr = np.ones_like(tex_x)
    tau = np.zeros_like(tex_x)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (far - t0) / dt
    n = np.where(x > 0, np.minimum(np.ceil(x), F32(p.dvr_max_steps)), F32(0)).astype(F32)
    n = np.where(hit, n, F32(0))
    dq = [dt * idr[i] for i in range(3)]
    q0 = [fma(t0, idr[i], ip[i]) - F32(0.5) for i in range(3)]
    done_all = np.zeros_like(hit)
    samples = tf_samples = 0
    k = 0
    while k < max_iter:
        alive = (F32(k) < n) & ~done_all
        if not alive.any():
            break
        samples += int(alive.sum())
        q = [fma(F32(k), dq[i], q0[i]) for i in range(3)]
        dens = vol.trilinear_q(p.volume_density_scale, *q)
        dn = dens * F32(p.volume_inv_maj)
        tf_samples += int((alive & ~((dn < F32(p.sample_range[0])) | (dn > F32(p.sample_range[1])))).sum())
        rgba = NP.transfer(tf, L, p.sample_range, dn)
        a = np.where(alive, rgba[..., 3], F32(0))
        pos_a = a > 0
        tau_n = fma(a * F32(p.volume_maj), dt, tau)
        Tn = np.exp(-tau_n.astype(np.float64)).astype(F32)
        dT = np.where(pos_a, Tr - Tn, F32(0))
        if T is not None:
            dT = dT * shadow_lookup(T, stride, *q, ilo, ihi)
        for c in range(3):
            C[c] = np.where(pos_a, fma(dT, rgba[..., c], C[c]), C[c])
        Tr = np.where(pos_a, Tn, Tr)
        tau = np.where(pos_a, tau_n, tau)
        done = pos_a & (tau >= F32(p.dvr_ert_tau))
        Tr = np.where(done, F32(0), Tr)
        done_all |= done
        k += 1
    nl = [-F32(p.light_dir[i]) for i in range(3)]
    cdot = _gmax(fma(d[2], nl[2], fma(d[1], nl[1], d[0] * nl[0])), zero)
    s = np.clip(np.power(cdot.astype(np.float64), 300.0), 0, 1).astype(F32)
    env = F32(p.env_strength) * fma(s, F32(4), F32(0.01))
    out = np.zeros((H, W, 4), dtype=F32)
    for c in range(3):
        Lc = C[c] * F32(p.dvr_gain[c])
        if p.show_environment > 0:
            Lc = np.where(Tr > 0, fma(Tr, env, Lc), Lc)
        out[..., c] = Lc
    out[..., 3] = 1
    return out, samples, tf_samples
