"""NumPy restatement of the distance field and the margins (DESIGN.md section 2 "Distances and margins"; vx_distance.hpp).

Masks are (Z, Y, X) bool arrays, spacings (s_x, s_y, s_z), fields (Z, Y, X) float32 of SQUARED distances.  Every operation is
a float32 NumPy operation, one rounding each, so the figures below are the definition's own bits:

    term(n, s)   fl32(p * p), p = fl32(fl32(n) * s)
    brute        D2(i) = min over the source voxels j of fl32(fl32(t_x + t_y) + t_z): the definition, one candidate at a time
    separable    the x, the y and the z pass, each a plain minimum over every candidate of the line
    windowed     the same passes over the cap's windows only (W_a = the largest n with t_a(n) <= R2), every partial above
                 the cap pruned to +inf on the way -- what the device does
    field        the same minimum by the cheapest exact route (an index-scan x pass, the cap's windows, scans that end once
                 term(n) has reached the largest value left); the tests' reference

brute == separable == windowed (after the cap) is asserted on small masks by tests/test_distance_host.py; the GPU tests
compare the device with `field`."""
import numpy as np

F32 = np.float32
INF = F32(np.inf)
OPS = ("grow", "shrink", "open", "close")


def term(n, s):
    p = np.asarray(n).astype(F32) * F32(s)
    return p * p


def cap2(r):
    """R2 = fl32(fl32(r) * fl32(r)); inf stays inf"""
    with np.errstate(over="ignore"):
        return F32(r) * F32(r)


def window(s, r2, L):
    """the largest n <= L - 1 with term(n, s) <= r2"""
    ok = np.nonzero(term(np.arange(L), s) <= r2)[0]
    return int(ok.max())


def capped(d2, r2):
    return np.where(d2 <= r2, d2, INF).astype(F32)


def brute(S, spacing, r=np.inf):
    """the definition: one candidate at a time over the whole volume, then the cap"""
    Z, Y, X = S.shape
    out = np.full(S.shape, INF, dtype=F32)
    tx, ty, tz = (term(np.arange(n), s) for n, s in zip((X, Y, Z), spacing))
    ax, ay, az = np.arange(X), np.arange(Y), np.arange(Z)
    for z, y, x in zip(*np.nonzero(S)):
        cand = (tx[np.abs(ax - x)][None, None, :] + ty[np.abs(ay - y)][None, :, None]) + tz[np.abs(az - z)][:, None, None]
        np.minimum(out, cand, out=out)
    return capped(out, cap2(r))


def _sl(axis, s):
    return tuple(s if a == axis else slice(None) for a in range(3))


def line_pass(g, axis, s, w=None, r2=None, stop=False):
    """out(j) = min over j' on the line of fl32(g(j') + term(|j - j'|, s)); w: only |j - j'| <= w; r2: results above it read inf;
    stop: end once term(n) has reached the largest value left (fl32(g + t) >= t: no later candidate can be smaller)"""
    L = g.shape[axis]
    out = g.copy()
    for n in range(1, (L - 1 if w is None else min(w, L - 1)) + 1):
        t = term(n, s)
        if stop and t >= out.max():
            break
        hi, lo = _sl(axis, slice(n, None)), _sl(axis, slice(None, L - n))
        out[hi] = np.minimum(out[hi], g[lo] + t)
        out[lo] = np.minimum(out[lo], g[hi] + t)
    return out if r2 is None else capped(out, r2)


def _start(S):
    return np.where(S, F32(0), INF).astype(F32)


def separable(S, spacing, r=np.inf):
    g = _start(S)
    for axis, s in ((2, spacing[0]), (1, spacing[1]), (0, spacing[2])):
        g = line_pass(g, axis, s)
    return capped(g, cap2(r))


def windowed(S, spacing, r):
    r2 = cap2(r)
    g = _start(S)
    for axis, s in ((2, spacing[0]), (1, spacing[1]), (0, spacing[2])):
        g = line_pass(g, axis, s, w=window(s, r2, S.shape[axis]), r2=r2)
    return g


def x_pass_by_index(S, sx):
    """term(n) of the distance n to the nearest set voxel of the x row, found by index scans"""
    X = S.shape[2]
    far = 4 * X
    idx = np.broadcast_to(np.arange(X), S.shape)
    left = np.maximum.accumulate(np.where(S, idx, -far), axis=2)
    right = np.minimum.accumulate(np.where(S, idx, far)[:, :, ::-1], axis=2)[:, :, ::-1]
    n = np.minimum(idx - left, right - idx)
    return np.where(n < X, term(np.minimum(n, X), sx), INF).astype(F32)


def field(S, spacing, r=np.inf):
    """the tests' reference: D2 of S under the cap r, by the cheapest exact route -- the index-scan x pass, the cap's windows
    with partials above the cap pruned, and scans that end once no candidate can be smaller"""
    r2 = cap2(r)
    g = capped(x_pass_by_index(S, spacing[0]), r2)
    for axis, s in ((1, spacing[1]), (0, spacing[2])):
        g = line_pass(g, axis, s, w=window(s, r2, S.shape[axis]), r2=r2, stop=True)
    return g


def source(M, side):
    return M if side == "outside" else ~M


def stats(d2, S, r=np.inf):
    """finite, max_d2 and argmax (x, y, z) as VxDistanceResult defines them; d2 is capped already"""
    fin = d2 <= cap2(r)
    fin &= np.isfinite(d2)
    cand = fin & ~S
    if not cand.any():
        return int(fin.sum()), 0.0, (0, 0, 0)
    k = int(np.argmax(np.where(cand, d2, F32(-1))))
    z, y, x = np.unravel_index(k, d2.shape)
    return int(fin.sum()), float(d2[z, y, x]), (int(x), int(y), int(z))


def grow(M, r, spacing, f=field):
    d2 = f(M, spacing, r)
    return (d2 <= cap2(r)) & np.isfinite(d2)


def shrink(M, r, spacing, f=field):
    d2 = f(~M, spacing, r)
    return M & ~((d2 <= cap2(r)) & np.isfinite(d2))


def margin(M, op, r, spacing, band=None, f=field):
    """the four margin ops; band: the predicate mask P of GROW's band form, M | (GROW(M) & P)"""
    if op == "grow":
        g = grow(M, r, spacing, f)
        return g if band is None else M | (g & band)
    assert band is None
    if op == "shrink":
        return shrink(M, r, spacing, f)
    if op == "close":
        return shrink(grow(M, r, spacing, f), r, spacing, f)
    if op == "open":
        return grow(shrink(M, r, spacing, f), r, spacing, f)
    raise ValueError(op)
