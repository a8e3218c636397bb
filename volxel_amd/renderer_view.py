"""The views of `Volxel3DRenderer` beside the accumulated render (vx_api_view.hip): slices and slabs, first-hit isosurfaces
and picking.  A mixin: the renderer supplies _lib, _ctx, _check, _out and bind_uniforms."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _abi, _checks


class ViewMixin:
    def slice(self, sp, reduce: str = "mean", display: str | None = None, window=None):
        """A slice or thick slab of the volume (vx_slice; planes from volxel_amd.mpr).  reduce: "mean", "max" or "min" over the
        sp.slab_samples samples; display: None, "grey" (window = (value shown black, value shown white)) or "tf" (the transfer
        function, premultiplied by its alpha).  Binds the current uniforms first (the densities use their density scale).
        Returns the (H, W) float32 values, row 0 = y = 0, or (values, the (H, W, 4) uint8 display) when a display is asked."""
        if not isinstance(sp, _abi.VxSliceParams):
            raise TypeError("sp must be a VxSliceParams (volxel_amd.mpr builds them)")
        if reduce not in _abi.SLICE_REDUCE:
            raise ValueError(f"reduce must be one of {sorted(_abi.SLICE_REDUCE)}, not {reduce!r}")
        if display not in _abi.SLICE_DISPLAY:
            raise ValueError(f"display must be None, 'grey' or 'tf', not {display!r}")
        q = _abi.VxSliceParams.from_buffer_copy(sp)
        W, H, _ = _checks.slice_spec(q)
        if display == "grey":
            w = np.asarray(window if window is not None else (), dtype=np.float64).reshape(-1)
            if w.size != 2 or not np.isfinite(w.astype(np.float32)).all() or not np.float32(w[1]) > np.float32(w[0]):
                raise ValueError(f"display 'grey' needs window = (black, white) with black < white, not {window!r}")
            q.window[0], q.window[1] = float(w[0]), float(w[1])
        elif window is not None:
            raise ValueError("window applies to display 'grey' only")
        q.reduce = _abi.SLICE_REDUCE[reduce]
        q.display = _abi.SLICE_DISPLAY[display]
        self.bind_uniforms()
        values = np.empty((H, W), dtype=np.float32)
        rgba = np.empty((H, W, 4), dtype=np.uint8) if display is not None else None
        self._check(self._lib.vx_slice(self._ctx, C.byref(q), values.ctypes.data,
                                       rgba.ctypes.data if rgba is not None else None))
        return values if rgba is None else (values, rgba)

    def slice_stats(self):
        """(samples, kernel_ms) of the last slice: W * H * slab_samples and its HIP-event time"""
        return self._out("vx_slice_stats", C.c_uint64, C.c_double)

    def isosurface(self, iso: float, color=(1.0, 1.0, 1.0), phong=None, refine: int = 8, skip: bool = True, window=None):
        """The shaded first-hit isosurface d = iso of the current view (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): DVR's
        rays and samples, `refine` bisection steps, Blinn-Phong on `color` with phong = (ka, kd, ks, shininess) (default: the
        settings' phong).  skip: range skipping (same bits).  window = (x0, y0, x1, y1) of the render size (x0 <= x < x1, GL rows:
        y = 0 is the bottom row) or None for the whole image.  Binds the current uniforms first.  Returns (rgba, hit), both
        (h, w, 4) float32 over the window, row 0 = y0: rgba alpha 1 on a hit and all 0 on a miss; hit = (world x, y, z, t) or
        (0, 0, 0, -1) on a miss."""
        q = _abi.VxIsoParams()
        iso32 = np.float32(iso)
        if not np.isfinite(iso32):
            raise ValueError(f"iso must be finite, not {iso!r}")
        col = np.asarray(color, dtype=np.float64).reshape(-1)
        if col.size != 3 or not np.isfinite(col.astype(np.float32)).all():
            raise ValueError(f"color must be three finite values, not {color!r}")
        ph = np.asarray(self.settings.phong if phong is None else phong, dtype=np.float64).reshape(-1)
        if ph.size != 4 or not np.isfinite(ph.astype(np.float32)).all():
            raise ValueError(f"phong must be four finite values (ka, kd, ks, shininess), not {phong!r}")
        if ph[3] < 0:
            raise ValueError(f"shininess must be >= 0, not {ph[3]}")
        q.refine = _checks.integer(refine, 0, _abi.ISO_MAX_REFINE,
                                   f"refine must be an integer 0 .. {_abi.ISO_MAX_REFINE}, not {refine!r}")
        if skip not in (True, False, 0, 1):
            raise ValueError(f"skip must be True or False, not {skip!r}")
        W, H = int(self.width), int(self.height)
        if window is None:
            x0, y0, x1, y1 = 0, 0, W, H
        else:
            w = tuple(window)
            if len(w) != 4 or any(isinstance(a, bool) or int(a) != a for a in w):
                raise ValueError(f"window must be four integers (x0, y0, x1, y1), not {window!r}")
            x0, y0, x1, y1 = (int(a) for a in w)
            if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
                raise ValueError(f"window {window!r} is empty or outside the render size {W} x {H}")
        q.iso = float(iso32)
        q.color[0], q.color[1], q.color[2] = (float(a) for a in col)
        q.ka, q.kd, q.ks, q.shininess = (float(a) for a in ph)
        q.skip = 1 if skip else 0
        q.window[0], q.window[1], q.window[2], q.window[3] = x0, y0, x1, y1
        self.bind_uniforms()
        rgba = np.empty((y1 - y0, x1 - x0, 4), dtype=np.float32)
        hit = np.empty((y1 - y0, x1 - x0, 4), dtype=np.float32)
        self._check(self._lib.vx_isosurface(self._ctx, C.byref(q), rgba.ctypes.data, hit.ctypes.data))
        return rgba, hit

    def pick(self, x: int, y: int, iso: float, refine: int = 16):
        """the world point (x, y, z) where the ray of pixel (x, y) (GL rows: y = 0 is the bottom row) first reaches density iso,
        or None when it misses: a one-pixel isosurface window"""
        _, hit = self.isosurface(iso, refine=refine, window=(x, y, x + 1, y + 1))
        h = hit[0, 0]
        return None if h[3] < 0 else tuple(float(a) for a in h[:3])

    def iso_stats(self):
        """(rays, hits, samples, refine_samples, skipped, kernel_ms) of the last isosurface"""
        return self._out("vx_iso_stats", *[C.c_uint64] * 5, C.c_double)
