"""The argument checks that several renderer methods share, as pure functions: each returns the value in the form the C
structs take, or raises the ValueError of the method that asked.  Nothing here touches the device."""
from __future__ import annotations

import math

import numpy as np

from . import _abi


def integer(x, lo: int, hi: int, message: str, whole_floats: bool = True) -> int:
    """x as an int in lo .. hi, or ValueError(message).  A bool never passes; a float with a whole value (2.0) passes unless
    whole_floats is False, which asks for an int or a NumPy integer."""
    whole = int(x) == x if whole_floats else isinstance(x, (int, np.integer))
    if isinstance(x, bool) or not whole or not lo <= int(x) <= hi:
        raise ValueError(message)
    return int(x)


def voxel(name: str, v, ext) -> tuple:
    """the voxel v = (x, y, z) inside the index extent; `name` is what the caller's argument is called"""
    t = tuple(v)
    if len(t) != 3 or any(isinstance(a, bool) or int(a) != a for a in t):
        raise ValueError(f"{name} must be three integer voxel indices (x, y, z), not {v!r}")
    if not all(0 <= int(a) < e for a, e in zip(t, ext)):
        raise ValueError(f"{name} {v!r} is outside the index extent {tuple(ext)}")
    return tuple(int(a) for a in t)


def band(lo, hi):
    """(lo, hi) as float32 with lo <= hi; hi = inf stands for the largest float32"""
    lo32 = np.float32(lo)
    hi32 = np.float32(np.finfo(np.float32).max) if hi == math.inf else np.float32(hi)
    if not (np.isfinite(lo32) and np.isfinite(hi32)):
        raise ValueError(f"lo and hi must be finite (hi may be inf), not {lo!r}, {hi!r}")
    if lo32 > hi32:
        raise ValueError(f"lo = {lo!r} > hi = {hi!r}")
    return lo32, hi32


def connectivity(c) -> int:
    if c not in (6, 26) or isinstance(c, bool):
        raise ValueError(f"connectivity must be 6 or 26, not {c!r}")
    return int(c)


def spacing(sp, transform) -> tuple:
    """the voxel spacing (s_x, s_y, s_z) as three finite float32 > 0; None: the norms of the columns of transform[:3, :3]
    (the grid's own units: mm for DICOM), cast to float32"""
    if sp is None:
        sp = np.linalg.norm(np.asarray(transform, dtype=np.float64)[:3, :3], axis=0)
    try:
        t = tuple(np.float32(a) for a in sp)
    except (TypeError, ValueError):
        t = ()
    if len(t) != 3 or not all(np.isfinite(a) and a > 0 for a in t):
        raise ValueError(f"spacing must be three finite numbers > 0 (x, y, z), not {sp!r}")
    return tuple(float(a) for a in t)


def distance(name: str, r, allow_inf: bool) -> float:
    """a radius or a cap r > 0 as float32; finite unless allow_inf (max_distance = inf: no cap)"""
    if isinstance(r, bool) or not isinstance(r, (int, float, np.integer, np.floating)):
        raise ValueError(f"{name} must be a number > 0, not {r!r}")
    r32 = np.float32(r)
    if not r32 > 0 or (np.isinf(r32) and not (allow_inf and r == math.inf)):
        raise ValueError(f"{name} must be {'> 0 (inf: no cap)' if allow_inf else 'finite and > 0'}, not {r!r}")
    return float(r32)


def slot(s, name: str = "slot") -> int:
    """a slot of the segment store: an int 0 .. SEGMENT_SLOTS - 1 (no bool, no float, no string)"""
    return integer(s, 0, _abi.SEGMENT_SLOTS - 1,
                   f"{name} must be an integer 0 .. {_abi.SEGMENT_SLOTS - 1}, not {s!r}", whole_floats=False)


def slots(ss) -> tuple:
    """the slot list of a label map: 1 .. SEGMENT_SLOTS different slots, in the order given"""
    try:
        t = tuple(ss)
    except TypeError:
        raise ValueError(f"slots must be a sequence of slots, not {ss!r}") from None
    if not 1 <= len(t) <= _abi.SEGMENT_SLOTS:
        raise ValueError(f"slots must list 1 .. {_abi.SEGMENT_SLOTS} slots, not {len(t)}")
    t = tuple(slot(s, "slots: every entry") for s in t)
    if len(set(t)) != len(t):
        raise ValueError(f"slots must not list a slot twice, as {list(t)!r} does")
    return t


def hist_source(source) -> tuple:
    """(VxHistSource, slot) of a histogram's `source`: "volume", "segment" or an int slot of the segment store"""
    if isinstance(source, str) and source in ("volume", "segment"):
        return _abi.HIST_SOURCES[source], 0
    message = f"source must be 'volume', 'segment' or an integer slot 0 .. {_abi.SEGMENT_SLOTS - 1}, not {source!r}"
    if isinstance(source, str):
        raise ValueError(message)
    return _abi.HIST_SOURCES["slot"], integer(source, 0, _abi.SEGMENT_SLOTS - 1, message, whole_floats=False)


def hist_bins(bins) -> int:
    return integer(bins, 1, _abi.HIST_MAX_BINS, f"bins must be an integer 1 .. {_abi.HIST_MAX_BINS}, not {bins!r}",
                   whole_floats=False)


def hist_range(r) -> tuple:
    """(lo, hi) of a histogram's range as float32 with lo < hi, both finite"""
    try:
        lo, hi = (np.float32(a) for a in r)
    except (TypeError, ValueError):
        raise ValueError(f"range must be (lo, hi), two finite numbers with lo < hi, not {r!r}") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and lo < hi):
        raise ValueError(f"range must be (lo, hi), two finite numbers with lo < hi, not {r!r}")
    return float(lo), float(hi)


def ranks(ks, n=None) -> tuple:
    """the 0-based ranks of an order statistic: a sequence of integers, 0 .. n - 1 once the size n of the region is known"""
    try:
        t = tuple(ks)
    except TypeError:
        raise ValueError(f"ranks must be a sequence of integers, not {ks!r}") from None
    if n is None:
        return tuple(integer(k, 0, 2 ** 64 - 1, f"ranks: every entry must be an integer >= 0, not {k!r}", whole_floats=False)
                     for k in t)
    return tuple(integer(k, 0, n - 1, f"ranks: every entry must be an integer 0 .. {n - 1} (the region has {n} voxels), "
                                      f"not {k!r}", whole_floats=False) for k in t)


def percentiles(q) -> tuple:
    """(values, scalar) of a percentile argument: a number or a sequence of numbers in [0, 100]"""
    scalar = isinstance(q, (int, float, np.integer, np.floating)) and not isinstance(q, bool)
    try:
        t = (q,) if scalar else tuple(q)
    except TypeError:
        t = (None,)
    for a in t:
        if isinstance(a, bool) or not isinstance(a, (int, float, np.integer, np.floating)) or not 0.0 <= float(a) <= 100.0:
            raise ValueError(f"q must be a number or a sequence of numbers in [0, 100], not {q!r}")
    return tuple(float(a) for a in t), scalar


def box(b, ext):
    """(lo, hi) of box = ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices inside the index extent; None: all of it"""
    if b is None:
        return (0, 0, 0), tuple(e - 1 for e in ext)
    try:
        blo, bhi = (tuple(v) for v in b)
    except (TypeError, ValueError):
        raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)), not {b!r}") from None
    if len(blo) != 3 or len(bhi) != 3 or any(isinstance(a, bool) or int(a) != a for a in blo + bhi):
        raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not {b!r}")
    blo, bhi = tuple(int(a) for a in blo), tuple(int(a) for a in bhi)
    if not all(0 <= a <= b1 < e for a, b1, e in zip(blo, bhi, ext)):
        raise ValueError(f"box {b!r} is empty or outside the index extent {tuple(ext)}")
    return blo, bhi


def slice_spec(sp):
    """(W, H, slab samples) of a VxSliceParams whose size, slab_samples and vectors the device will accept"""
    W, H, N = int(sp.size[0]), int(sp.size[1]), int(sp.slab_samples)
    if not (1 <= W <= _abi.SLICE_MAX_SIZE and 1 <= H <= _abi.SLICE_MAX_SIZE):
        raise ValueError(f"slice size must be 1 .. {_abi.SLICE_MAX_SIZE} per side, not {W} x {H}")
    if not 1 <= N <= _abi.SLICE_MAX_SAMPLES:
        raise ValueError(f"slab_samples must be 1 .. {_abi.SLICE_MAX_SAMPLES}, not {N}")
    for name in ("origin", "du", "dv", "dn"):
        if not np.isfinite(np.asarray(getattr(sp, name)[:], dtype=np.float32)).all():
            raise ValueError(f"slice {name} must be finite")
    return W, H, N
