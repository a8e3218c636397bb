"""The histogram contract restated in NumPy (include/volxel_hip.h "histograms", DESIGN.md section 2 "Histograms"): the two bin
rules with np.float32 operations, the radix select they give, the moments and Otsu's split.  Every function takes the float32
densities of the region as a flat array; the tests select the region."""
import math

import numpy as np

F32 = np.float32
PASSES = ((0, 11), (11, 11), (22, 10))   # (prefix_bits, key_bits): 32 bits in three passes


def inv_of(bins, lo, hi):
    """fl32(fl32(B) / fl32(hi - lo))"""
    return F32(bins) / (F32(hi) - F32(lo))


def linear_bins(d, bins, lo, hi):
    """the counter of every density: its bin, `bins` for below, bins + 1 for above"""
    d = np.asarray(d, dtype=F32)
    lo, hi = F32(lo), F32(hi)
    inv = inv_of(bins, lo, hi)
    t = ((d - lo).astype(F32) * inv).astype(F32)
    inside = (d >= lo) & (d <= hi)
    b = np.minimum(np.where(inside, t, F32(0)).astype(np.uint32), np.uint32(bins - 1)).astype(np.int64)
    return np.where(d < lo, bins, np.where(d > hi, bins + 1, b))


def linear(d, bins, lo, hi):
    """(counts uint64[bins], below, above) of VX_HIST_LINEAR"""
    c = np.bincount(linear_bins(d, bins, lo, hi), minlength=bins + 2).astype(np.uint64)
    return c[:bins], int(c[bins]), int(c[bins + 1])


def order_key(d):
    """seg_order_key: the bits of a float32 as a uint32 with the order of the floats (-0 below +0)"""
    u = np.ascontiguousarray(d, dtype=F32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def key_float(key):
    """the float32 of an order key"""
    key = int(key)
    u = key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff
    return np.array([u], dtype=np.uint32).view(F32)[0]


def key_pass(d, prefix, p, b):
    """(counts uint64[2^b], below, above) of VX_HIST_KEY"""
    key = order_key(d).astype(np.uint64)
    top = key >> np.uint64(32 - p) if p else np.zeros_like(key)
    b_ = (key >> np.uint64(32 - p - b)) & np.uint64((1 << b) - 1)
    mine = top == prefix
    c = np.bincount(b_[mine].astype(np.int64), minlength=1 << b).astype(np.uint64)
    return c, int((top < prefix).sum()), int((top > prefix).sum())


def select(d, k, pass_fn=None):
    """the k-th smallest of d (0-based) from three key passes; pass_fn(prefix, p, b) -> (counts, below, above) stands in for
    key_pass where the counts come from somewhere else"""
    pass_fn = pass_fn or (lambda prefix, p, b: key_pass(d, prefix, p, b))
    prefix = 0
    for p, b in PASSES:
        c, below, _ = pass_fn(prefix, p, b)
        j = int(np.searchsorted(np.cumsum(c.astype(np.int64)), k - below, side="right"))
        assert j < (1 << b), "the rank lies beyond the region"
        prefix = (prefix << b) | j
    return key_float(prefix)


def lower_rank(q, n):
    """the rank of np.percentile(method="lower"): floor(q / 100 * (n - 1)) in float64"""
    return int(math.floor(float(q) / 100.0 * (n - 1)))


def moments(d):
    """count, d_min, d_max and the float64 sums of d and d * d (each product rounded once, then an exact sum)"""
    d = np.asarray(d, dtype=F32)
    if d.size == 0:
        return dict(count=0, d_min=0.0, d_max=0.0, d_sum=0.0, d_sum2=0.0)
    d64 = d.astype(np.float64)
    return dict(count=int(d.size), d_min=float(d.min()), d_max=float(d.max()), d_sum=math.fsum(d64), d_sum2=math.fsum(d64 * d64))


def mean_std(m):
    n = m["count"]
    if not n:
        return math.nan, math.nan
    return m["d_sum"] / n, math.sqrt(max(0.0, (m["d_sum2"] - m["d_sum"] ** 2 / n) / n))


def edges(bins, lo, hi):
    lo, hi = float(F32(lo)), float(F32(hi))
    return lo + np.arange(bins + 1, dtype=np.float64) * (hi - lo) / bins


def otsu_variances(counts, lo=0.0, hi=1.0):
    """the between-class variance w0 w1 (mu0 - mu1)^2 of every split k = 0 .. B - 2 (classes: bins 0 .. k and k + 1 .. B - 1), bin
    centres standing for the bins, one split at a time in float64; 0 where a class is empty"""
    c = [float(x) for x in counts]
    B = len(c)
    e = edges(B, lo, hi)
    centre = [(e[i] + e[i + 1]) / 2 for i in range(B)]
    out = []
    for k in range(B - 1):
        w0, w1 = sum(c[:k + 1]), sum(c[k + 1:])
        if w0 == 0 or w1 == 0:
            out.append(0.0)
            continue
        m0 = sum(a * x for a, x in zip(c[:k + 1], centre[:k + 1])) / w0
        m1 = sum(a * x for a, x in zip(c[k + 1:], centre[k + 1:])) / w1
        out.append(w0 * w1 * (m0 - m1) ** 2)
    return out


def otsu(counts, lo=0.0, hi=1.0):
    """(k, threshold): the split of the largest variance, the lowest k among equal ones, and the upper edge of its bin; (-1, nan)
    with fewer than two non-empty bins"""
    if sum(1 for x in counts if x) < 2:
        return -1, math.nan
    v = otsu_variances(counts, lo, hi)
    k = max(range(len(v)), key=lambda i: (v[i], -i))
    return k, float(edges(len(counts), lo, hi)[k + 1])
