"""NumPy restatement of the segment views (vx_set_segment_view, DESIGN.md section 2 "Segment views"): a masked image is, bit for
bit, the image of a volume whose hidden voxels decode to +0.  MaskedVolume wraps NpVolume so that brick() returns 0 where a voxel
is hidden (ONLY: not in the segment; HIDE: in it); the existing march code then restates masked DVR (np_oracle.dvr_image), the
projections (projection_ref.projection_image) and the isosurface (iso_ref.isosurface) with no change of its own.  Masks are
(Z, Y, X) bool arrays over the index extent, as Volxel3DRenderer.segment_mask returns them."""
import contextlib

import numpy as np

from oracle import np_oracle as NP
from tests import iso_ref as IR
from tests import projection_ref as PR

F32 = np.float32
VIEWS = ("only", "hide")


def visible(mask, view):
    """the voxels a view keeps: the segment under ONLY, its complement under HIDE, everything under OFF"""
    mask = np.asarray(mask, dtype=bool)
    if view == "off":
        return np.ones_like(mask)
    if view == "only":
        return mask
    if view == "hide":
        return ~mask
    raise ValueError(view)


class MaskedVolume(NP.NpVolume):
    """NpVolume of `grid` whose voxel i reads +0 where keep[z, y, x] is False (outside the volume: 0, as before)"""

    def __init__(self, grid, keep):
        super().__init__(grid)
        self.keep = np.asarray(keep, dtype=bool)
        assert self.keep.shape == tuple(int(e) for e in self.ext[::-1]), (self.keep.shape, self.ext)

    def brick(self, x, y, z):
        v = super().brick(x, y, z)
        x, y, z = [np.asarray(a, dtype=np.int64) for a in (x, y, z)]
        ok = (x >= 0) & (y >= 0) & (z >= 0) & (x < self.ext[0]) & (y < self.ext[1]) & (z < self.ext[2])
        k = self.keep[np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)]
        return np.where(ok & ~k, F32(0), v)


@contextlib.contextmanager
def _masked(grid, keep):
    """while inside: np_oracle.NpVolume(grid) -- what dvr_image and projection_image build -- is the masked volume"""
    plain = NP.NpVolume

    def make(g):
        return MaskedVolume(g, keep) if g is grid else plain(g)

    NP.NpVolume = make
    try:
        yield
    finally:
        NP.NpVolume = plain


def dvr_image(p, grid, tf, L, mask, view):
    """np_oracle.dvr_image (jitter off) of the masked volume: (image (H, W, 4), samples)"""
    with _masked(grid, visible(mask, view)):
        return NP.dvr_image(p, grid, tf, L)


def projection_image(p, grid, tf, L, mask, view, minip=False):
    """projection_ref.projection_image of the masked volume"""
    with _masked(grid, visible(mask, view)):
        return PR.projection_image(p, grid, tf, L, minip=minip)


def isosurface(p, grid, iso, mask, view, **kw):
    """iso_ref.isosurface of the masked volume (no range skipping: a masked isosurface never skips)"""
    return IR.isosurface(p, MaskedVolume(grid, visible(mask, view)), iso, **kw)


def blobs():
    """(A+B, A alone, B alone) as u16 stacks [z, y, x] of 64^3: two noisy solid balls, A in bricks x 0-2, B in bricks x 4-6,
    brick column x 3 empty; every voxel of a ball is well above 0, every other voxel 0"""
    Z, Y, X = 64, 64, 64
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    rng = np.random.default_rng(11)
    noise = rng.integers(0, 1500, size=(Z, Y, X))
    a = ((x - 11.5) ** 2 + (y - 11.5) ** 2 + (z - 11.0) ** 2 < 10.0 ** 2) & (x < 24)
    b = ((x - 44.0) ** 2 + (y - 12.5) ** 2 + (z - 12.0) ** 2 < 9.0 ** 2) & (x >= 32)
    va = np.where(a, 1500 + noise, 0).astype(np.uint16)
    vb = np.where(b, 2200 + noise, 0).astype(np.uint16)
    # one shared maximum: both stacks normalise by the same largest value, so A decodes alike in A+B and in A alone
    m = np.uint16(4000)
    va[11, 11, 11] = m
    vb[12, 12, 44] = m
    return va + vb, va, vb
