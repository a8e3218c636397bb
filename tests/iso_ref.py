"""NumPy restatement of the first-hit isosurfaces (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): DVR's rays and samples with
the pixel-centre ray and start offset 1/2 (projection_ref.rays), d_k = trilinear(q_k) * volume_inv_maj (NpVolume.trilinear_q
reproduces the device's densities bit for bit), the first k < n with d_k >= iso, `refine` fp32 bisection steps on the sample
parameter, t = fma(s*, dt, t0) and w = fma(t, d, o).  Every one of those steps is exact or correctly rounded, so the device's hit
buffer and counters must match to the bit.  The shading restates Phong's central difference in fp32 (exact, so the flat-gradient
decision is too) and the normal and Blinn-Phong terms with IEEE 1/sqrt and pow where the device uses its hardware rsq / log2 /
exp2: the colour matches to Phong's tolerance, 1e-5."""
import numpy as np

from oracle import np_oracle as NP
from tests.projection_ref import rays
from tests.shadow_ref import _slab

F32 = np.float32
fma = NP.fma
MAX_REFINE = 16


def world_rays(p):
    """per pixel (H, W): the world ray o (3 arrays), d (3 arrays) and t0, dt of the march contract -- the operations of
    projection_ref.rays, which gives q0, dq and n of the same rays"""
    W, H = p.res[0], p.res[1]
    px, py = np.meshgrid(np.arange(W), np.arange(H))
    tex_x = (px.astype(F32) + F32(0.5)) / F32(W)
    tex_y = (py.astype(F32) + F32(0.5)) / F32(H)
    one, zero = np.ones_like(tex_x), np.zeros_like(tex_x)
    mm = NP._mat_mul
    cw = mm(p.camera_view_inv[:], zero, zero, zero, one)
    o = [cw[i] / cw[3] for i in range(3)]
    vp = mm(p.camera_proj_inv[:], fma(tex_x, F32(2), F32(-1)), fma(tex_y, F32(2), F32(-1)), zero, one)
    vv = [vp[i] / vp[3] for i in range(3)]
    wp = mm(p.camera_view_inv[:], vv[0], vv[1], vv[2], one)
    d = [wp[i] / wp[3] - o[i] for i in range(3)]
    if getattr(p, "camera_ortho", 0):
        npt = mm(p.camera_proj_inv[:], fma(tex_x, F32(2), F32(-1)), fma(tex_y, F32(2), F32(-1)), -one, one)
        wo = mm(p.camera_view_inv[:], npt[0] / npt[3], npt[1] / npt[3], npt[2] / npt[3], one)
        o = [wo[i] / wo[3] for i in range(3)]
        wd = mm(p.camera_view_inv[:], zero, zero, -one, zero)
        d = [wd[i] for i in range(3)]
    dd = fma(d[2], d[2], fma(d[1], d[1], d[0] * d[0]))
    inv = F32(1) / np.sqrt(dd)
    d = [a * inv for a in d]
    _, near, _ = _slab(o, d, p.volume_aabb_min, p.volume_aabb_max)
    idr = mm(p.density_transform_inv[:], d[0], d[1], d[2], zero)
    il = fma(idr[2], idr[2], fma(idr[1], idr[1], idr[0] * idr[0]))
    dt = F32(p.dvr_step_voxels) / np.sqrt(il)
    t0 = fma(F32(0.5), dt, near)
    return o, d, t0, dt


def trilinear_cell(vol, scale, i, f):
    """the device's trilinear_cell: cells i (3 int arrays) with fractions f (3 float32 arrays), NpVolume.trilinear_q's mixes"""
    B = vol.brick

    def mix(a, b, t):
        return fma(b, t, a * (F32(1) - t))

    lx0 = mix(B(i[0], i[1], i[2]), B(i[0] + 1, i[1], i[2]), f[0])
    lx1 = mix(B(i[0], i[1] + 1, i[2]), B(i[0] + 1, i[1] + 1, i[2]), f[0])
    hx0 = mix(B(i[0], i[1], i[2] + 1), B(i[0] + 1, i[1], i[2] + 1), f[0])
    hx1 = mix(B(i[0], i[1] + 1, i[2] + 1), B(i[0] + 1, i[1] + 1, i[2] + 1), f[0])
    return F32(scale) * mix(mix(lx0, lx1, f[1]), mix(hx0, hx1, f[1]), f[2])


def _dot(a, b):
    return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0]))


def isosurface(p, grid, iso, color=(1.0, 1.0, 1.0), phong=(0.3, 0.7, 0.4, 32.0), refine=8, window=None, bound=None):
    """(rgba (h, w, 4), hit (h, w, 4), counts, per_ray) over window = (x0, y0, x1, y1) (default: the whole image), row 0 = y0.
    counts: {rays, hits, samples, refine_samples, skipped}; per_ray: k, found, cap, n, s (= s*), samples, skipped per pixel.
    bound: None, or a function of the cell-frame positions (3 arrays) giving the upper density bound of their macro cell -- a
    sample whose bound is below iso is skipped (counted in `skipped`), as range skipping does; the hits do not depend on it."""
    W, H = p.res[0], p.res[1]
    x0, y0, x1, y1 = window if window is not None else (0, 0, W, H)
    hit, n, q0, dq = rays(p)
    o, d, t0, dt = world_rays(p)
    sl = (slice(y0, y1), slice(x0, x1))
    hit, n, t0, dt = hit[sl], n[sl], t0[sl], dt[sl]
    q0, dq, o, d = [[a[sl] for a in v] for v in (q0, dq, o, d)]
    vol = grid if isinstance(grid, NP.NpVolume) else NP.NpVolume(grid)
    iso, scale, inv_maj = F32(iso), F32(p.volume_density_scale), F32(p.volume_inv_maj)

    def pos(s):
        return [fma(s, dq[a], q0[a]) for a in range(3)]

    def density(s):
        return vol.trilinear_q(scale, *pos(s)) * inv_maj

    shape = n.shape
    found = np.zeros(shape, dtype=bool)
    kf = np.zeros(shape, dtype=F32)
    samples = np.zeros(shape, dtype=np.int64)
    skipped = np.zeros(shape, dtype=np.int64)
    k = 0
    while True:
        live = ~found & (F32(k) < n)
        if not live.any():
            break
        s = np.full(shape, F32(k))
        dk = density(s)
        skip = np.zeros(shape, dtype=bool) if bound is None else (bound(*pos(s)) < iso)
        skipped += live & skip
        ev = live & ~skip
        samples += ev
        now = ev & (dk >= iso)
        found |= now
        kf = np.where(now, F32(k), kf)
        k += 1
    cap = found & (kf == F32(0))
    lo, hi = kf - F32(1), kf.copy()
    for _ in range(int(refine)):
        mid = F32(0.5) * (lo + hi)
        up = density(mid) >= iso
        hi = np.where(up, mid, hi)
        lo = np.where(up, lo, mid)
    s = np.where(found & ~cap, hi, kf).astype(F32)
    t = fma(s, dt, t0)
    hit_out = np.zeros(shape + (4,), dtype=F32)
    hit_out[..., 3] = -1
    for a in range(3):
        hit_out[..., a] = np.where(found, fma(t, d[a], o[a]), F32(0))
    hit_out[..., 3] = np.where(found, t, F32(-1))

    # Phong's central difference in the cell frame of q(s*), scaled by density_transform_inv's diagonal
    q = pos(s)
    fl = [np.floor(a) for a in q]
    fr = [a - b for a, b in zip(q, fl)]
    ci = [b.astype(np.int64) for b in fl]
    m = [F32(p.density_transform_inv[i]) for i in (0, 5, 10)]
    g = []
    for a in range(3):
        up = [c + (1 if b == a else 0) for b, c in enumerate(ci)]
        dn = [c - (1 if b == a else 0) for b, c in enumerate(ci)]
        g.append((trilinear_cell(vol, scale, up, fr) - trilinear_cell(vol, scale, dn, fr)) * m[a])
    g2 = _dot(g, g)
    shaded = ~cap & (g2 > F32(1e-12))
    inv = (1.0 / np.sqrt(np.where(shaded, g2, F32(1)).astype(np.float64))).astype(F32)
    nrm = [np.where(shaded, g[a] * -inv, -d[a]) for a in range(3)]
    nl = [-F32(p.light_dir[a]) for a in range(3)]
    hv = [nl[a] - d[a] for a in range(3)]
    hinv = F32(1) / np.sqrt(_dot(hv, hv))
    hv = [a * hinv for a in hv]
    ka, kd, ks, shin = (F32(x) for x in phong)
    ndl = np.maximum(F32(0), _dot(nrm, nl))
    ndh = np.maximum(F32(0), _dot(nrm, hv))
    diff = fma(kd, ndl, ka)
    pw = np.ones(shape) if shin == 0 else np.power(ndh.astype(np.float64), float(shin))
    spec = (ks * pw.astype(F32)).astype(F32)
    rgba = np.zeros(shape + (4,), dtype=F32)
    for a in range(3):
        rgba[..., a] = np.where(found, fma(F32(color[a]), diff, spec), F32(0))
    rgba[..., 3] = np.where(found, F32(1), F32(0))
    counts = {"rays": int(hit.sum()), "hits": int(found.sum()), "samples": int(samples.sum()),
              "refine_samples": int(refine) * int((found & ~cap).sum()), "skipped": int(skipped.sum())}
    return rgba, hit_out, counts, {"k": kf, "found": found, "cap": cap, "n": n, "s": s, "samples": samples,
                                   "skipped": skipped}


def bound_table(lib, grid, p):
    """the upper density bound of range skipping as a function of cell-frame positions: the projections' table
    (vx_debug_build_projection_bounds, pure CPU), indexed by the mask cell floor(q) + 1 clamped to extent + 7 per axis"""
    import ctypes as C
    rng = np.asarray(grid.range, dtype=np.uint16).view(np.uint32)
    bc = (C.c_uint32 * 3)(*grid.indirection_size)
    level, dims = C.c_uint32(), (C.c_uint32 * 3)()
    assert lib.vx_debug_build_projection_bounds(rng.ctypes.data, bc, C.byref(p), None, C.byref(level), dims) == 0
    out = np.empty(2 * dims[0] * dims[1] * dims[2], dtype=F32)
    assert lib.vx_debug_build_projection_bounds(rng.ctypes.data, bc, C.byref(p), out.ctypes.data, C.byref(level), dims) == 0
    hi = out.reshape(dims[2], dims[1], dims[0], 2)[..., 1]
    sh = 3 + int(level.value)
    cmax = [int(e) + 7 for e in grid.index_extent]

    def bound(qx, qy, qz):
        c = []
        for a, q in enumerate((qx, qy, qz)):
            m = np.floor(q).astype(np.int64) + 1
            m = np.where(m < 0, cmax[a], np.minimum(m, cmax[a]))       # the device's unsigned compare: negative -> clamped
            c.append(m >> sh)
        return hi[c[2], c[1], c[0]]
    return bound
