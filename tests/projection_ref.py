"""NumPy restatement of the intensity projections (VX_MODE_MIP / VX_MODE_MINIP, DESIGN.md section 2 "projections"), jitter off:
DVR's rays and samples (np_oracle.dvr_image's ray set-up and march contract), density d_k = trilinear(q_k) * volume_inv_maj
(NpVolume.trilinear_q reproduces the device's densities bit for bit), m = max_k d_k or min_k d_k, pixel TF(m) * alpha with
alpha 1.  Max and min are exact, so the device must match this to the bit."""
import numpy as np

from oracle import np_oracle as NP
from tests.shadow_ref import _slab

F32 = np.float32
fma = NP.fma


def rays(p):
    """per pixel (H, W): hit, n, q0 (3 arrays), dq (3 arrays) of the march contract with the pixel-centre ray and start offset
    1/2 (dvr_jitter = 0)"""
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
    ip = mm(p.density_transform_inv[:], cam[0], cam[1], cam[2], one)
    idr = mm(p.density_transform_inv[:], d[0], d[1], d[2], zero)
    il = fma(idr[2], idr[2], fma(idr[1], idr[1], idr[0] * idr[0]))
    dt = F32(p.dvr_step_voxels) / np.sqrt(il)
    t0 = fma(F32(0.5), dt, near)
    with np.errstate(divide="ignore", invalid="ignore"):
        x = (far - t0) / dt
    n = np.where(x > 0, np.minimum(np.ceil(x), F32(p.dvr_max_steps)), F32(0)).astype(F32)
    n = np.where(hit, n, F32(0))
    dq = [dt * idr[i] for i in range(3)]
    q0 = [fma(t0, idr[i], ip[i]) - F32(0.5) for i in range(3)]
    return hit, n, q0, dq


def projection_image(p, grid, tf, L, minip=False, window=None):
    """(image (H, W, 4), sum of n over the rays, tf_samples, rays).  window = (x0, y0, x1, y1): only those pixels are computed
    (the others stay (0, 0, 0, 1)); the sums cover the window."""
    hit, n, q0, dq = rays(p)
    H, W = n.shape
    sel = np.zeros((H, W), dtype=bool)
    if window is None:
        sel[:] = True
    else:
        x0, y0, x1, y1 = window
        sel[y0:y1, x0:x1] = True
    idx = np.nonzero(sel)
    n_s = n[idx]
    q0_s = [a[idx] for a in q0]
    dq_s = [a[idx] for a in dq]
    vol = NP.NpVolume(grid)
    m = np.full(n_s.shape, np.inf if minip else -np.inf, dtype=F32)
    k = 0
    while True:
        alive = F32(k) < n_s
        if not alive.any():
            break
        a = np.nonzero(alive)
        q = [fma(F32(k), dq_s[i][a], q0_s[i][a]) for i in range(3)]
        dn = vol.trilinear_q(p.volume_density_scale, *q) * F32(p.volume_inv_maj)
        m[a] = np.minimum(m[a], dn) if minip else np.maximum(m[a], dn)
        k += 1
    has = n_s > 0
    rgba = NP.transfer(tf, L, p.sample_range, np.where(has, m, F32(0)))
    out = np.zeros((H, W, 4), dtype=F32)
    out[..., 3] = 1
    for c in range(3):
        out[..., c][idx] = np.where(has, rgba[..., c] * rgba[..., 3], F32(0))
    return out, int(n_s.astype(np.int64).sum()), int(has.sum()), int(hit[idx].sum())
