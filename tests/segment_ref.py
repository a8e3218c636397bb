"""NumPy / SciPy restatement of the segmentation (vx_segment, DESIGN.md section 2 "Segmentation"): voxel densities
d(i) = (volume_density_scale * v(i)) * volume_inv_maj in fp32 from NpVolume, the predicate with its box, the component of the seed
(scipy.ndimage.label, or an independent masked-dilation fixpoint), the statistics, the packed mask and the slice overlay.  Arrays
are indexed [z, y, x]; seeds, boxes and bboxes are (x, y, z)."""
import math

import numpy as np
from scipy import ndimage

from oracle import np_oracle as NP
from tests import slice_ref as SR

F32 = np.float32
Q_MAX = F32(16777216.0)


def densities(grid, scale, inv_maj):
    """d over the index extent, (Z, Y, X) fp32: two fp32 products, in that order"""
    vol = grid if isinstance(grid, NP.NpVolume) else NP.NpVolume(grid)
    X, Y, Z = (int(e) for e in vol.ext)
    out = np.empty((Z, Y, X), dtype=F32)
    y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    for z in range(Z):
        v = vol.brick(x, y, np.full_like(x, z))
        out[z] = (F32(scale) * v).astype(F32) * F32(inv_maj)
    return out


def predicate(d, lo, hi, box=None):
    """lo <= d <= hi (inclusive, fp32) inside box = ((x0, y0, z0), (x1, y1, z1)) (inclusive); None: everywhere"""
    p = (F32(lo) <= d) & (d <= F32(hi))
    if box is not None:
        (x0, y0, z0), (x1, y1, z1) = box
        inside = np.zeros_like(p)
        inside[z0:z1 + 1, y0:y1 + 1, x0:x1 + 1] = True
        p &= inside
    return p


def component(p, seed, conn):
    """the connected component of p holding seed (x, y, z): scipy.ndimage.label with the 6 / 26 structure"""
    x, y, z = seed
    if not p[z, y, x]:
        return np.zeros_like(p)
    lab, _ = ndimage.label(p, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
    return lab == lab[z, y, x]


def _dilate(m, conn):
    """one step of the 6- or 26-neighbourhood dilation, by shifted copies (no scipy)"""
    out = m.copy()
    Z, Y, X = m.shape
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                if (dx, dy, dz) == (0, 0, 0) or (conn == 6 and abs(dx) + abs(dy) + abs(dz) != 1):
                    continue
                src = m[max(0, -dz):Z - max(0, dz), max(0, -dy):Y - max(0, dy), max(0, -dx):X - max(0, dx)]
                out[max(0, dz):Z - max(0, -dz), max(0, dy):Y - max(0, -dy), max(0, dx):X - max(0, -dx)] |= src
    return out


def fixpoint(p, seed, conn, max_steps=None):
    """the same component as a masked-dilation fixpoint from the seed voxel (small volumes)"""
    x, y, z = seed
    m = np.zeros_like(p)
    if not p[z, y, x]:
        return m
    m[z, y, x] = True
    steps = 0
    while max_steps is None or steps < max_steps:
        n = _dilate(m, conn) & p
        steps += 1
        if np.array_equal(n, m):
            break
        m = n
    return m


def stats(mask, d):
    """count, bbox (x, y, z) inclusive, min, max and math.fsum of d over the mask; (0, (0,0,0), (0,0,0), 0, 0, 0) when empty"""
    n = int(mask.sum())
    if n == 0:
        return {"count": 0, "bbox_lo": (0, 0, 0), "bbox_hi": (0, 0, 0), "d_min": 0.0, "d_max": 0.0, "d_sum": 0.0}
    z, y, x = np.nonzero(mask)
    v = d[mask]
    return {"count": n, "bbox_lo": (int(x.min()), int(y.min()), int(z.min())), "bbox_hi": (int(x.max()), int(y.max()), int(z.max())),
            "d_min": float(v.min()), "d_max": float(v.max()), "d_sum": math.fsum(v.astype(np.float64).tolist())}


def packed(mask):
    """one bit per voxel over (Z, Y, X) in C order, LSB first"""
    return np.packbits(np.asarray(mask, dtype=bool).ravel(), bitorder="little")


def unpacked(bits, shape):
    return np.unpackbits(np.asarray(bits, dtype=np.uint8), bitorder="little")[:int(np.prod(shape))].astype(bool).reshape(shape)


def overlay(sp, mask):
    """(H, W) bool: for any slab sample s, the nearest voxel floor(q + 0.5f) of the slice's fp32 position q (clamped to
    +-2^24) lies in the volume and in mask"""
    b = SR.bases(sp)
    dn = [F32(v) for v in sp.dn[:]]
    Z, Y, X = mask.shape
    out = np.zeros(b[0].shape, dtype=bool)
    for s in range(int(sp.slab_samples)):
        q = [np.clip(NP.fma(F32(s), dn[a], b[a]), -Q_MAX, Q_MAX) for a in range(3)]
        i = [np.floor((qa + F32(0.5)).astype(F32)).astype(np.int64) for qa in q]
        ok = (i[0] >= 0) & (i[0] < X) & (i[1] >= 0) & (i[1] < Y) & (i[2] >= 0) & (i[2] < Z)
        hit = np.zeros_like(ok)
        hit[ok] = mask[i[2][ok], i[1][ok], i[0][ok]]
        out |= hit
    return out
