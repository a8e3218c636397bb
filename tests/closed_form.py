"""Float64 geometry for the closed-form pins (tests/test_analytic_pins.py, tests/test_closed_form_pins.py), written from the scene
alone: the grid's spacing and extent, the camera's position, look-at point and fov, the clip box as fractions of the grid's box,
the light.  Nothing here reads VxParams or calls a restatement: the transform chain of viewer.ts:1089-1099 (scene.Volume.normalise)
and the camera of SURVEY Appendix C (tan(fov/2), look-at basis) are written out by hand."""
import math

import numpy as np

FOVY = math.pi / 3.0                    # scene.ts:55


def homogeneous_grid(oracle, n=32, spacing=(1.0, 1.0, 1.0)):
    """an n^3 stack of constant value with one brighter voxel in the far corner: every other voxel normalises to exactly 1/2"""
    vox = np.full((n, n, n), 2000, dtype=np.uint16)
    vox[n - 1, n - 1, n - 1] = 4000
    return oracle.BrickGrid(vox, tuple(spacing))


def make_pin_scene(grid, width, height, mode, eye, look, clip_lo, clip_hi, light, **kw):
    """the uniforms of the scene (tests.common.make_scene): no environment, the light as given"""
    from tests.common import make_scene
    return make_scene(grid, width, height, mode, cam_pos=tuple(eye), look_at=tuple(look), clip_min=tuple(clip_lo),
                      clip_max=tuple(clip_hi), show_environment=False, use_env=False, light_dir=tuple(light), **kw)


def world_scale(extent, spacing):
    """S = the longest side of the grid's box before normalisation: world = spacing * (index - extent / 2) / S"""
    e, s = np.asarray(extent, float), np.asarray(spacing, float)
    return float((e * s).max())


def index_to_world(idx, extent, spacing):
    """index position (..., 3) -> world (..., 3): the grid transform diag(spacing), then centre at the origin, longest side 1"""
    e, s = np.asarray(extent, float), np.asarray(spacing, float)
    return s * (np.asarray(idx, float) - e / 2.0) / world_scale(e, s)


def world_to_index(w, extent, spacing):
    e, s = np.asarray(extent, float), np.asarray(spacing, float)
    return np.asarray(w, float) * world_scale(e, s) / s + e / 2.0


def index_per_world(spacing, extent):
    """d(index)/d(world) per axis: a world-space direction d maps to idir = d * this"""
    s = np.asarray(spacing, float)
    return world_scale(extent, s) / s


def world_box(extent, spacing, clip_lo, clip_hi):
    """the clipped box in world space: the fractions clip_lo / clip_hi of the grid's index extent (volume.ts:32-37)"""
    e = np.asarray(extent, float)
    return (index_to_world(np.asarray(clip_lo, float) * e, e, spacing),
            index_to_world(np.asarray(clip_hi, float) * e, e, spacing))


def camera_basis(eye, look):
    z = (np.asarray(eye, float) - np.asarray(look, float))
    z /= np.linalg.norm(z)
    x = np.cross([0.0, 1.0, 0.0], z)
    x /= np.linalg.norm(x)
    return x, np.cross(z, x), z


def camera_rays(eye, look, width, height, sub=1):
    """world-space camera rays through the pixel grid (closed form, row 0 = GL's bottom row); sub x sub positions per pixel
    covering the support of the reference's jitter (+-1 pixel, triangular weights, fragment.frag:146).  Returns (dirs, weights)."""
    aspect, th = width / height, math.tan(FOVY / 2.0)
    x, y, z = camera_basis(eye, look)
    offs = np.array([0.0]) if sub == 1 else (np.arange(sub) + 0.5) / sub * 2.0 - 1.0     # in pixels
    wts = np.array([1.0]) if sub == 1 else (1.0 - np.abs(offs))
    wts = wts / wts.sum()
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    dirs, weights = [], []
    for oy, wy in zip(offs, wts):
        for ox, wx in zip(offs, wts):
            nx = ((px + 0.5 + ox) / width) * 2.0 - 1.0
            ny = ((py + 0.5 + oy) / height) * 2.0 - 1.0
            d = x[None, None, :] * (nx * aspect * th)[..., None] + y[None, None, :] * (ny * th)[..., None] - z[None, None, :]
            dirs.append(d / np.linalg.norm(d, axis=-1, keepdims=True))
            weights.append(wx * wy)
    return dirs, weights


def slab(o, d, lo, hi):
    """(near, far) of rays o + t d against the box [lo, hi], near clamped at 0; a zero direction component means the slab of
    that axis holds the whole ray when o lies inside it and none of it otherwise (no inf * 0)"""
    o, d = np.broadcast_arrays(np.asarray(o, float), np.asarray(d, float))
    lo, hi = np.asarray(lo, float), np.asarray(hi, float)
    zero = d == 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        t0, t1 = (lo - o) / d, (hi - o) / d
    inside = (o >= lo) & (o <= hi)
    tmin = np.where(zero, np.where(inside, -np.inf, np.inf), np.minimum(t0, t1))
    tmax = np.where(zero, np.where(inside, np.inf, -np.inf), np.maximum(t0, t1))
    near = np.maximum(0.0, tmin.max(axis=-1))
    far = tmax.min(axis=-1)
    return near, far


def chord(o, w, lo, hi):
    """length of the part of the ray o + t w (t >= 0, |w| = 1) inside the box: the optical path toward the light is sigma times this"""
    near, far = slab(o, w, lo, hi)
    return np.maximum(far - near, 0.0)


def decode(oracle, grid, extent=None):
    """the decoded voxels (z, y, x) as the device sees them (vxo_lookup_density_brick, tap by tap) over `extent` (default: the
    data's dimensions rounded up to whole bricks; every voxel beyond them decodes to 0)"""
    L = oracle.lib()
    vol = oracle.make_volume(grid)
    nz, ny, nx = grid.voxels.shape
    ex, ey, ez = extent if extent is not None else [8 * ((n + 7) // 8) for n in (nx, ny, nz)]
    dec = np.zeros((ez, ey, ex), dtype=np.float64)
    for z in range(ez):
        for y in range(ey):
            for x in range(ex):
                dec[z, y, x] = L.vxo_lookup_density_brick(vol, x, y, z)
    return dec


def trilinear(dec, qx, qy, qz):
    """float64 trilinear interpolation of dec (z, y, x) at cell-frame positions q (voxel i has its centre at q = i); taps beyond
    the array read 0"""
    q = [np.asarray(a, float) for a in (qx, qy, qz)]
    c = [np.floor(a) for a in q]
    f = [a - b for a, b in zip(q, c)]
    i = [b.astype(np.int64) for b in c]
    nz, ny, nx = dec.shape

    def tap(x, y, z):
        ok = (x >= 0) & (y >= 0) & (z >= 0) & (x < nx) & (y < ny) & (z < nz)
        return np.where(ok, dec[np.where(ok, z, 0), np.where(ok, y, 0), np.where(ok, x, 0)], 0.0)

    out = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                w = (f[0] if dx else 1 - f[0]) * (f[1] if dy else 1 - f[1]) * (f[2] if dz else 1 - f[2])
                out = out + w * tap(i[0] + dx, i[1] + dy, i[2] + dz)
    return out


def neighbour_steps(dec, lo=None, hi=None):
    """per axis (x, y, z) the largest |difference| of neighbouring voxels of dec (zero padding included) inside the voxel block
    [lo, hi) (x, y, z; default all, one padding voxel either side): a Lipschitz bound of the trilinear along that axis there"""
    pad = np.pad(dec, 1)
    lo = np.zeros(3, int) if lo is None else np.asarray(lo, int) + 1
    hi = np.array(pad.shape[::-1]) if hi is None else np.asarray(hi, int) + 1
    lo, hi = np.clip(lo, 0, np.array(pad.shape[::-1])), np.clip(hi, 0, np.array(pad.shape[::-1]))
    blk = pad[lo[2]:hi[2], lo[1]:hi[1], lo[0]:hi[0]]
    return np.array([np.abs(np.diff(blk, axis=a)).max() if blk.shape[a] > 1 else 0.0 for a in (2, 1, 0)])
