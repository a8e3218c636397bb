"""NumPy restatement of the segment store's set operations, comparison and label map (DESIGN.md section 2 "Segment store";
vx_segstore.hpp).

Masks are (Z, Y, X) bool arrays over the index extent, A the current segment and B the mask of a slot; voxels are reported
(x, y, z); spacings are (s_x, s_y, s_z).

    combine      the five ops: A | B, A & B, A & ~B, A ^ B and ~A (over the whole index extent, padding included)
    counts       |A|, |B|, |A & B|; dice = 2 and / (a + b), jaccard = and / (a + b - and), nan when both sets are empty
    directed     the directed Hausdorff value of `own` towards `other`: the max over the voxels of `own` of the squared distance
                 field of `other` (tests/distance_ref.py `field`: float32, the definition's own bits), with the first voxel in
                 C order that attains it.  `own` empty: 0.0 and (0, 0, 0).  `other` empty and `own` not: the field is +inf
                 everywhere, so the value is +inf and the voxel the first of `own`
    labelmap     uint8 labels, k + 1 for the first listed mask that holds the voxel, 0 for none; overlaps = the voxels that more
                 than one listed mask holds
"""
import math

import numpy as np

from tests import distance_ref as DR

F32 = np.float32
OPS = ("union", "intersect", "subtract", "xor", "invert")


def combine(op, A, B=None):
    if op == "invert":
        return ~A
    if op == "union":
        return A | B
    if op == "intersect":
        return A & B
    if op == "subtract":
        return A & ~B
    if op == "xor":
        return A ^ B
    raise ValueError(op)


def counts(A, B):
    return int(A.sum()), int(B.sum()), int((A & B).sum())


def dice(a, b, n):
    return 2 * n / (a + b) if a + b else math.nan


def jaccard(a, b, n):
    return n / (a + b - n) if a + b else math.nan


def directed_from_field(own, d2):
    """(value, (x, y, z)) of the field d2 over the voxels of `own`: the largest, the first in C order among equal ones"""
    if not own.any():
        return F32(0.0), (0, 0, 0)
    flat = np.flatnonzero(own.ravel())
    v = d2.ravel()[flat]
    k = int(flat[int(np.argmax(v))])          # argmax returns the first of equal maxima; flat ascends in C order
    z, y, x = np.unravel_index(k, own.shape)
    return F32(d2[z, y, x]), (int(x), int(y), int(z))


def directed(own, other, spacing, f=DR.field):
    return directed_from_field(own, f(other, spacing))


def labelmap(masks):
    """(labels, overlaps) of the masks in list order"""
    labels = np.zeros(masks[0].shape, dtype=np.uint8)
    held = np.zeros(masks[0].shape, dtype=np.uint8)
    for k, m in enumerate(masks):
        labels[m & (labels == 0)] = k + 1
        held += m
    return labels, int((held > 1).sum())
