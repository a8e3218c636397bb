"""Multiplanar reformation: the planes of `Volxel3DRenderer.slice` (vx_slice, DESIGN.md section 2 "Slices").

Every helper returns a `VxSliceParams` with one slab sample, reduce = mean and no display; `Volxel3DRenderer.slice` sets
those three.  Positions are in the cell frame of the march contract (q = index position - 1/2), so voxel i has its centre
at q = i.

`axial`, `coronal` and `sagittal` are the index-space planes z = k, y = j and x = i through voxel centres, one pixel per
voxel, covering the grid's index extent.  Patient orientation (the DICOM ImageOrientationPatient tag) is not modelled:
"axial" names the planes of constant slice index of the series as it was stacked, and so on for the other two.
"""
from __future__ import annotations

import numpy as np

from . import _abi


def _extent(src):
    """index extent of a renderer (its uploaded volume), a scene.Grid or a BrickGridMessage"""
    vol = getattr(src, "volume", None)
    if vol is not None:
        src = vol.grid
    e = getattr(src, "index_extent", None)
    if e is None:
        raise ValueError("expected a renderer with a volume, a Grid or a BrickGridMessage")
    return [int(x) for x in e]


def _params(origin, du, dv, dn, size, samples=1):
    sp = _abi.VxSliceParams()
    for name, vec in (("origin", origin), ("du", du), ("dv", dv), ("dn", dn)):
        getattr(sp, name)[:] = [float(x) for x in np.asarray(vec, dtype=np.float64).astype(np.float32)]
    sp.size[0], sp.size[1] = int(size[0]), int(size[1])
    sp.slab_samples = int(samples)
    sp.reduce = _abi.SLICE_MEAN
    sp.display = _abi.SLICE_NONE
    sp.window[0], sp.window[1] = 0.0, 1.0
    return sp


def _index(name, i, n):
    if int(i) != i or not 0 <= i < n:
        raise ValueError(f"{name} must be a voxel index in [0, {n}), not {i}")
    return int(i)


def axial(src, k: int):
    """the plane z = k: pixel (x, y) shows voxel (x, y, k); W x H = extent x x extent y; dn = +z"""
    e = _extent(src)
    k = _index("k", k, e[2])
    return _params((0, 0, k), (1, 0, 0), (0, 1, 0), (0, 0, 1), (e[0], e[1]))


def coronal(src, j: int):
    """the plane y = j: pixel (x, y) shows voxel (x, j, y); W x H = extent x x extent z; dn = +y"""
    e = _extent(src)
    j = _index("j", j, e[1])
    return _params((0, j, 0), (1, 0, 0), (0, 0, 1), (0, 1, 0), (e[0], e[2]))


def sagittal(src, i: int):
    """the plane x = i: pixel (x, y) shows voxel (i, x, y); W x H = extent y x extent z; dn = +x"""
    e = _extent(src)
    i = _index("i", i, e[0])
    return _params((i, 0, 0), (0, 1, 0), (0, 0, 1), (1, 0, 0), (e[1], e[2]))


def oblique(renderer, center, normal, up, pixel_size: float, size, thickness: float = 0.0, samples: int = 1):
    """A plane in world coordinates (the camera's frame): centred on `center`, facing `normal`, `up` giving the direction of
    +y on the image (its part along the normal is dropped); +x = up x normal.  `size` = (W, H) pixels of `pixel_size` world
    units.  `samples` slab samples are spaced thickness / samples apart along the normal and centred on the plane.

    The plane is mapped to the cell frame through density_transform_inv of the renderer's current params, in float64, and
    each vector is rounded to fp32 once -- anisotropic voxel spacing scales du, dv and dn per axis."""
    W, H = int(size[0]), int(size[1])
    if not (1 <= W <= _abi.SLICE_MAX_SIZE and 1 <= H <= _abi.SLICE_MAX_SIZE):
        raise ValueError(f"size must be 1 .. {_abi.SLICE_MAX_SIZE} per side, not {W} x {H}")
    samples = int(samples)
    if not 1 <= samples <= _abi.SLICE_MAX_SAMPLES:
        raise ValueError(f"samples must be 1 .. {_abi.SLICE_MAX_SAMPLES}, not {samples}")
    if not (np.isfinite(pixel_size) and pixel_size > 0):
        raise ValueError(f"pixel_size must be > 0, not {pixel_size}")
    if not (np.isfinite(thickness) and thickness >= 0):
        raise ValueError(f"thickness must be >= 0, not {thickness}")
    c = np.asarray(center, dtype=np.float64).reshape(3)
    n = np.asarray(normal, dtype=np.float64).reshape(3)
    up = np.asarray(up, dtype=np.float64).reshape(3)
    if not (np.isfinite(c).all() and np.isfinite(n).all() and np.isfinite(up).all()):
        raise ValueError("center, normal and up must be finite")
    ln = np.linalg.norm(n)
    if ln == 0:
        raise ValueError("normal must not be zero")
    n = n / ln
    v = up - np.dot(up, n) * n
    lv = np.linalg.norm(v)
    if lv <= 1e-9 * max(np.linalg.norm(up), 1e-300):
        raise ValueError("up must not be parallel to the normal")
    v = v / lv
    u = np.cross(v, n)
    spacing = float(thickness) / samples
    o = c - (W - 1) / 2 * pixel_size * u - (H - 1) / 2 * pixel_size * v - (samples - 1) / 2 * spacing * n
    p = renderer._params if getattr(renderer, "_params", None) is not None else renderer.bind_uniforms()
    m = np.asarray(p.density_transform_inv[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T   # column major
    m3 = m[:3, :3]
    q0 = m3 @ o + m[:3, 3] - 0.5
    return _params(q0, m3 @ (pixel_size * u), m3 @ (pixel_size * v), m3 @ (spacing * n), (W, H), samples)


def overlay(rgba8, mask, color=(1.0, 0.0, 0.0), alpha: float = 0.5):
    """A segment overlay for display (pure NumPy): where `mask` (H, W) is True, each colour channel c of the (H, W, 3 or 4) uint8
    image becomes round((1 - alpha) * c + alpha * 255 * color); elsewhere, and in the alpha channel, the image is unchanged.
    color: three values in [0, 1]; alpha in [0, 1].  Returns a new array.  Renderer.slice_mask gives the mask of a slice."""
    img = np.asarray(rgba8)
    m = np.asarray(mask, dtype=bool)
    if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] not in (3, 4):
        raise ValueError(f"rgba8 must be an (H, W, 3 or 4) uint8 image, not {img.dtype} {img.shape}")
    if m.shape != img.shape[:2]:
        raise ValueError(f"mask must be {img.shape[:2]}, not {m.shape}")
    col = np.asarray(color, dtype=np.float64).reshape(-1)
    if col.size != 3 or not np.isfinite(col).all() or (col < 0).any() or (col > 1).any():
        raise ValueError(f"color must be three values in [0, 1], not {color!r}")
    a = float(alpha)
    if not 0.0 <= a <= 1.0:
        raise ValueError(f"alpha must be in [0, 1], not {alpha!r}")
    out = img.copy()
    rgb = out[..., :3].astype(np.float64)
    blend = np.floor((1.0 - a) * rgb + a * 255.0 * col + 0.5)
    out[..., :3] = np.where(m[..., None], np.clip(blend, 0, 255), rgb).astype(np.uint8)
    return out
