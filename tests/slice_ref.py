"""NumPy restatement of the slices (vx_slice, DESIGN.md section 2 "Slices"): sample positions as fma chains in fp32, densities
d_s = trilinear(q) * volume_inv_maj (NpVolume.trilinear_q reproduces the device's densities bit for bit), the reductions
looped over s in order in fp32, and the displays in fp32 operations.  Every step is exact or correctly rounded, so the device
must match this to the bit."""
import numpy as np

from oracle import np_oracle as NP

F32 = np.float32
fma = NP.fma
MEAN, MAX, MIN = 0, 1, 2
NONE, GREY, TF = 0, 1, 2
REDUCE_IDS = {"mean": MEAN, "max": MAX, "min": MIN}


def _v(sp, name):
    return [F32(x) for x in getattr(sp, name)[:]]


def bases(sp, window=None):
    """per pixel (H, W) or the window's pixels: fma(y, dv, fma(x, du, origin)) per axis"""
    W, H = int(sp.size[0]), int(sp.size[1])
    x0, y0, x1, y1 = window if window is not None else (0, 0, W, H)
    x, y = np.meshgrid(np.arange(x0, x1).astype(F32), np.arange(y0, y1).astype(F32))
    o, du, dv = _v(sp, "origin"), _v(sp, "du"), _v(sp, "dv")
    return [fma(y, dv[a], fma(x, du[a], o[a])) for a in range(3)]


def values(sp, grid, p, reduce=None, window=None):
    """the reduced values (H, W), or those of window = (x0, y0, x1, y1); reduce defaults to sp.reduce"""
    reduce = int(sp.reduce) if reduce is None else reduce
    vol = NP.NpVolume(grid) if not isinstance(grid, NP.NpVolume) else grid
    b = bases(sp, window)
    dn = _v(sp, "dn")
    N = int(sp.slab_samples)
    acc = None
    for s in range(N):
        q = [fma(F32(s), dn[a], b[a]) for a in range(3)]
        d = vol.trilinear_q(p.volume_density_scale, *q) * F32(p.volume_inv_maj)
        if acc is None:
            acc = d
        elif reduce == MEAN:
            acc = (acc + d).astype(F32)
        elif reduce == MAX:
            acc = np.fmax(acc, d)
        else:
            acc = np.fmin(acc, d)
    return (acc / F32(N)).astype(F32) if reduce == MEAN else acc


def _byte(c):
    """(uint8_t)(gl_clamp(c, 0, 1) * 255 + 0.5); gl_max(x, y) = x < y ? y : x, gl_min(x, y) = y < x ? y : x"""
    c = np.asarray(c, dtype=F32)
    c = np.where(c < F32(0), F32(0), c)
    c = np.where(F32(1) < c, F32(1), c)
    return (c * F32(255) + F32(0.5)).astype(F32).astype(np.uint8)


def display(v, sp, tf=None, L=None, sample_range=None, mode=None):
    """the RGBA8 display of the values v (..., 4); mode defaults to sp.display"""
    mode = int(sp.display) if mode is None else mode
    out = np.empty(v.shape + (4,), dtype=np.uint8)
    out[..., 3] = 255
    if mode == GREY:
        w0, w1 = F32(sp.window[0]), F32(sp.window[1])
        g = _byte((v - w0) / (w1 - w0))
        out[..., 0] = out[..., 1] = out[..., 2] = g
    elif mode == TF:
        rgba = NP.transfer(tf, L, sample_range, v)
        for c in range(3):
            out[..., c] = _byte(rgba[..., c] * rgba[..., 3])
    else:
        raise ValueError("no display")
    return out
