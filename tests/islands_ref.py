"""The islands of a mask (DESIGN.md section 2 "Islands"), restated twice: (a) scipy.ndimage.label with the 6- / 26-structure,
np.bincount, the first C-order index per label and a stable sort by -count -- SciPy numbers components by first appearance in C
order, so a stable sort IS the tie rule; (b) an independent NumPy fixpoint that peels one component after another from the first
remaining voxel (tests/segment_ref.fixpoint: masked dilation by shifted copies, no SciPy), so the reference does not rest on
SciPy alone.  Both return the same `Table`; the ops are filters of it."""
from dataclasses import dataclass

import numpy as np
from scipy import ndimage

from tests import segment_ref as SG


def structure(conn):
    if conn not in (6, 26):
        raise ValueError(conn)
    return ndimage.generate_binary_structure(3, 1 if conn == 6 else 3)


@dataclass
class Table:
    """canonical order: counts[k], anchors[k] = (x, y, z), bbox_lo / bbox_hi[k] = (x, y, z) inclusive; labels: (Z, Y, X) uint32,
    k + 1 on island k and 0 elsewhere"""
    counts: np.ndarray
    anchors: list
    bbox_lo: list
    bbox_hi: list
    labels: np.ndarray

    def __len__(self):
        return len(self.counts)

    def rows(self):
        return [(int(c), a, lo, hi) for c, a, lo, hi in zip(self.counts, self.anchors, self.bbox_lo, self.bbox_hi)]


def _table(lab, n, order_key=None):
    """lab: components numbered 1 .. n in order of first appearance in C order"""
    shape = lab.shape
    flat = lab.ravel()
    counts = np.bincount(flat, minlength=n + 1)[1:].astype(np.uint64)
    first = np.full(n + 1, flat.size, dtype=np.int64)
    idx = np.nonzero(flat)[0]
    np.minimum.at(first, flat[idx], idx)
    first = first[1:]
    if order_key is None:
        order = np.argsort(-counts.astype(np.int64), kind="stable")   # ties: first appearance = anchor ascending
    else:
        order = order_key(counts, first)
    rank = np.zeros(n + 1, dtype=np.uint32)
    rank[order + 1] = np.arange(1, n + 1, dtype=np.uint32)
    out = rank[lab]
    Z, Y, X = shape
    anchors, lo, hi = [], [], []
    boxes = ndimage.find_objects(lab.astype(np.int32), max_label=n) if n else []
    for k in order:
        i = int(first[k])
        anchors.append((i % X, (i // X) % Y, i // (X * Y)))
        sz, sy, sx = boxes[k]
        lo.append((sx.start, sy.start, sz.start))
        hi.append((sx.stop - 1, sy.stop - 1, sz.stop - 1))
    return Table(counts[order], anchors, lo, hi, out)


def scipy_islands(mask, conn):
    lab, n = ndimage.label(np.asarray(mask, dtype=bool), structure=structure(conn))
    return _table(lab, n)


def numpy_islands(mask, conn):
    """(b): peel the component of the first remaining voxel in C order until none is left (small volumes)"""
    rest = np.asarray(mask, dtype=bool).copy()
    Z, Y, X = rest.shape
    lab = np.zeros(rest.shape, dtype=np.int64)
    n = 0
    while True:
        idx = np.flatnonzero(rest)
        if idx.size == 0:
            break
        i = int(idx[0])
        comp = SG.fixpoint(rest, (i % X, (i // X) % Y, i // (X * Y)), conn)
        n += 1
        lab[comp] = n
        rest &= ~comp
    return _table(lab, n)


def islands(mask, conn):
    return scipy_islands(mask, conn)


def same(a, b):
    return (np.array_equal(a.counts, b.counts) and a.anchors == b.anchors and a.bbox_lo == b.bbox_lo and a.bbox_hi == b.bbox_hi
            and np.array_equal(a.labels, b.labels))


def _filter(t, keep):
    """the table and labels after keeping the islands keep[k]: the kept ones keep their relative order"""
    keep = np.asarray(keep, dtype=bool)
    new = np.zeros(len(t) + 1, dtype=np.uint32)
    new[1:][keep] = np.arange(1, int(keep.sum()) + 1, dtype=np.uint32)
    ks = [k for k in range(len(t)) if keep[k]]
    return Table(t.counts[keep], [t.anchors[k] for k in ks], [t.bbox_lo[k] for k in ks], [t.bbox_hi[k] for k in ks], new[t.labels])


def apply(mask, op, conn, keep=1, min_voxels=1, seed=None, table=None):
    """(new mask, table of the new mask, islands before, kept, largest) of one op"""
    t = islands(mask, conn) if table is None else table
    n = len(t)
    if op == "label":
        k = np.ones(n, dtype=bool)
    elif op == "keep_largest":
        k = np.arange(n) < keep
    elif op == "remove_small":
        k = t.counts >= np.uint64(min_voxels)
    elif op == "keep_at":
        x, y, z = seed
        k = np.arange(n) == int(t.labels[z, y, x]) - 1
    else:
        raise ValueError(op)
    new = _filter(t, k)
    return new.labels != 0, new, n, len(new), int(t.counts[0]) if n else 0


# ---- wrong references (negative controls of tests/test_islands_host.py) ------------------------------------------------------
def reversed_ties(mask, conn):
    """ties by anchor DESCENDING"""
    lab, n = ndimage.label(np.asarray(mask, dtype=bool), structure=structure(conn))
    return _table(lab, n, order_key=lambda c, f: np.lexsort((-f, -c.astype(np.int64))))


def conn18(mask):
    lab, n = ndimage.label(np.asarray(mask, dtype=bool), structure=ndimage.generate_binary_structure(3, 2))
    return _table(lab, n)


def brick_major_anchors(mask, conn):
    """the anchor = the first voxel in BRICK-major order (brick x fastest, then z, y, x inside the 8^3 brick) instead of C order"""
    t = scipy_islands(mask, conn)
    Z, Y, X = mask.shape
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    b = ((z >> 3) * (Y >> 3) + (y >> 3)) * (X >> 3) + (x >> 3)
    key = b * 512 + (z & 7) * 64 + (y & 7) * 8 + (x & 7)
    anchors = []
    for k in range(len(t)):
        sel = t.labels == k + 1
        i = int(np.argmin(np.where(sel, key, key.max() + 1)))
        anchors.append((i % X, (i // X) % Y, i // (X * Y)))
    order = sorted(range(len(t)), key=lambda k: (-int(t.counts[k]), key[anchors[k][2], anchors[k][1], anchors[k][0]]))
    rank = np.zeros(len(t) + 1, dtype=np.uint32)
    for new, k in enumerate(order):
        rank[k + 1] = new + 1
    return Table(t.counts[order], [anchors[k] for k in order], [t.bbox_lo[k] for k in order], [t.bbox_hi[k] for k in order],
                 rank[t.labels])
