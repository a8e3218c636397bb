"""Float64 geometry for the closed-form pins (tests/test_analytic_pins.py, tests/test_closed_form_pins.py), written from the scene
alone: the grid's spacing and extent, the camera's position, look-at point and fov, the clip box as fractions of the grid's box,
the light.  Nothing here reads VxParams or calls a restatement: the transform chain of viewer.ts:1089-1099 (scene.Volume.normalise)
and the camera of SURVEY Appendix C (tan(fov/2), look-at basis) are written out by hand."""
import math

import numpy as np

FOVY = math.pi / 3.0                    # scene.ts:55


def homogeneous_grid(oracle, n=32, spacing=(1.0, 1.0, 1.0)):
    """an n^3 stack of constant value with one brighter voxel in the far corner: every other voxel normalises to exactly 1/2
    and decodes to it, except in the brick of the brighter voxel: its u8 codes span [0, 1] (the brick's dilated window reaches the
    zero padding), and 1/2 decodes to 128/255 there"""
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


def ortho_rays(eye, look, width, height, half_height, near=0.1):
    """world-space rays of the orthographic camera (scene.ortho, near plane 0.1): each pixel centre's point on the near plane,
    all running along the camera's -z.  Returns (origins (H, W, 3), dirs (H, W, 3))"""
    x, y, z = camera_basis(eye, look)
    aspect = width / height
    py, px = np.meshgrid(np.arange(height), np.arange(width), indexing="ij")
    nx = ((px + 0.5) / width) * 2.0 - 1.0
    ny = ((py + 0.5) / height) * 2.0 - 1.0
    o = (np.asarray(eye, float) + x * (nx * aspect * half_height)[..., None] + y * (ny * half_height)[..., None]
         - z * near)
    return o, np.broadcast_to(-z, o.shape).copy()


def march_samples(o, d, lo, hi, ipw, step, max_steps, start=0.5):
    """the DVR march contract in float64: dt = step / |d * ipw| world units, t0 = near + start dt,
    n = min(ceil((far - t0) / dt), max_steps) samples (none unless the quotient is positive) at t0 + k dt.  Returns
    (dt, quotient (far - t0) / dt, n, valid (..., N), world positions (..., N, 3))"""
    o, d = np.broadcast_arrays(np.asarray(o, float), np.asarray(d, float))
    near, far = slab(o, d, lo, hi)
    dt = step / np.linalg.norm(d * np.asarray(ipw, float), axis=-1)
    t0 = near + start * dt
    x = (far - t0) / dt
    n = np.where(x > 0, np.minimum(np.ceil(np.where(x > 0, x, 0.0)), max_steps), 0).astype(np.int64)
    k = np.arange(max(int(n.max()), 1))
    valid = k < n[..., None]
    t = t0[..., None] + k * dt[..., None]
    return dt, x, n, valid, o[..., None, :] + t[..., None] * d[..., None, :]


def central_differences(dec, q):
    """(T(q), D) at cell-frame positions q (..., 3): T the float64 trilinear of dec and D[..., i] = T(c + e_i) - T(c - e_i),
    the trilinear of the cells one voxel either side along axis i with the sample's own fractions"""
    q = np.asarray(q, float)
    T = trilinear(dec, q[..., 0], q[..., 1], q[..., 2])
    D = []
    for a in range(3):
        e = np.zeros(3)
        e[a] = 1.0
        D.append(trilinear(dec, *np.moveaxis(q + e, -1, 0)) - trilinear(dec, *np.moveaxis(q - e, -1, 0)))
    return T, np.stack(D, axis=-1)


def blinn_phong(colour, n, light, h, ka, kd, ks, shininess):
    """Blinn-Phong of a TF colour (..., 3) with unit normals n (..., 3): colour (ka + kd max(0, n.l)) + ks max(0, n.h)^s,
    l = -light (the direction toward the light), h the half vector; spec is white, 0^0 = 1"""
    ndl = np.maximum(0.0, (n * -np.asarray(light, float)).sum(axis=-1))
    ndh = np.maximum(0.0, (n * h).sum(axis=-1))
    spec = ks * (np.ones_like(ndh) if shininess == 0 else ndh ** shininess)
    return colour * (ka + kd * ndl)[..., None] + spec[..., None]


def half_vector(light, d):
    """Blinn's h = normalize(l + v), l = -light toward the light, v = -d toward the eye"""
    h = -np.asarray(light, float) - np.asarray(d, float)
    return h / np.linalg.norm(h, axis=-1, keepdims=True)


def directional_environment(d, light, strength=1.0):
    """the background of the directional light without an environment map: strength (clamp(max(0, d.l)^300) 4 + 0.01)"""
    c = np.maximum(0.0, (np.asarray(d, float) * -np.asarray(light, float)).sum(axis=-1))
    return strength * (np.clip(c ** 300, 0.0, 1.0) * 4.0 + 0.01)
