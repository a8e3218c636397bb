"""The segment chain of `Volxel3DRenderer` (vx_api_segment.hip): seeded region growing and thresholds, edits, islands, the
distance field and the margins, the segment store with its set operations, comparison and label map, the masked views, the masks and voxel_index.  A mixin: the renderer supplies _lib, _ctx, _check, _out, _index_extent,
bind_uniforms and restart_rendering."""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _abi, _checks
from ._errors import VolxelError


@dataclass(frozen=True)
class Segment:
    """What Volxel3DRenderer.segment returns (VxSegmentResult): the voxel count, the inclusive bbox (x, y, z), min / max / sum
    (float64) / mean of the density over the segment (0, 0, 0 and nan when empty), the flood's rounds and brick visits (which may
    vary from run to run), whether it converged, and its volume: volume_grid = count * |det(grid.transform[:3, :3])| in the
    grid's own units (the voxel spacing: mm^3 for DICOM), volume_world = count * |det(density_transform[:3, :3])| in the
    scene's, where the volume is normalised to a unit box."""
    count: int
    bbox_lo: tuple
    bbox_hi: tuple
    d_min: float
    d_max: float
    d_sum: float
    mean: float
    rounds: int
    converged: bool
    brick_visits: int
    volume_grid: float
    volume_world: float


@dataclass(frozen=True)
class IslandSegment(Segment):
    """The `Segment` of the mask after keep_largest_islands / remove_small_islands / keep_island_at, with the op's own
    figures (VxIslandsResult): `islands` of the mask before the op, `kept` after it, `largest` = the voxel count of the
    largest island before the op (0 for an empty mask)."""
    islands: int = 0
    kept: int = 0
    largest: int = 0


class Islands:
    """What Volxel3DRenderer.islands returns: the islands of the current segment in canonical order (count descending, ties by
    the C-order index of the anchor ascending; island k has label k + 1).  count: how many; sizes: their voxel counts (uint64);
    table: one dict per island (label, count, anchor, bbox_lo, bbox_hi, each (x, y, z)); largest; segment: the `Segment` of the
    labelled mask; labels(): the dense (Z, Y, X) uint32 label volume, read from the device when asked (refused once the
    segment has changed)."""

    def __init__(self, renderer, res, rows, segment):
        self._renderer = renderer
        self.count = int(res.islands)
        self.largest = int(res.largest)
        self.segment = segment
        self.sizes = np.array([r.count for r in rows], dtype=np.uint64)
        self.table = [dict(label=int(r.label), count=int(r.count), anchor=tuple(r.anchor[:]), bbox_lo=tuple(r.bbox_lo[:]),
                           bbox_hi=tuple(r.bbox_hi[:])) for r in rows]

    def labels(self) -> np.ndarray:
        return self._renderer.island_labels()

    def __len__(self):
        return self.count


class SegmentDistance:
    """What Volxel3DRenderer.segment_distance returns (VxDistanceResult): `finite` = the voxels within the cap, `max_distance` =
    the largest distance within the cap over the voxels outside the source set (side "inside": the radius of the largest ball of
    voxel centres inside the segment) and `argmax` = (x, y, z), the first voxel in C order that attains it ((0, 0, 0) and 0.0
    when there is none); squared() and distance(): the (Z, Y, X) float32 field of squared distances and its square root, inf
    beyond the cap, read from the device when asked (refused once the segment has changed)."""

    def __init__(self, renderer, res, side, spacing, cap):
        self._renderer = renderer
        self.side, self.spacing, self.cap = side, spacing, cap
        self.finite = int(res.finite)
        self.max_d2 = float(res.max_d2)
        self.max_distance = float(np.sqrt(np.float32(res.max_d2)))
        self.argmax = tuple(res.argmax[:])

    def squared(self) -> np.ndarray:
        return self._renderer.distance_field()

    def distance(self) -> np.ndarray:
        return np.sqrt(self.squared())


@dataclass(frozen=True)
class SegmentComparison:
    """What Volxel3DRenderer.segment_compare returns (VxCompareResult), A the current segment and B the slot: count_a, count_b,
    count_and = |A|, |B|, |A & B|; dice = 2 and / (a + b) and jaccard = and / (a + b - and), nan when both sets are empty.  With
    hausdorff: d2_ab / d2_ba = the largest squared distance from a voxel of A to B / of B to A, hausdorff_ab / hausdorff_ba their
    float32 square roots, hausdorff the larger of the two, argmax_ab / argmax_ba = (x, y, z), the first voxel in C order that
    attains each; a direction whose own set is empty gives 0 and (0, 0, 0), one whose other set alone is empty inf and the first
    voxel of its own.  All of these are None when hausdorff was not asked for."""
    count_a: int
    count_b: int
    count_and: int
    dice: float
    jaccard: float
    d2_ab: float | None = None
    d2_ba: float | None = None
    hausdorff_ab: float | None = None
    hausdorff_ba: float | None = None
    hausdorff: float | None = None
    argmax_ab: tuple | None = None
    argmax_ba: tuple | None = None


@dataclass(frozen=True)
class Histogram:
    """What Volxel3DRenderer.histogram returns (vx_histogram, LINEAR): `counts` (uint64, one per bin), `edges` (float64,
    lo + k (hi - lo) / B for k = 0 .. B: nominal -- the fp32 rule of include/volxel_hip.h decides the bin), `below` / `above`
    (voxels with d < lo / d > hi), `count` = below + above + counts.sum() = the voxels of the region, and over ALL of the
    region: d_min, d_max, d_sum and d_sum2 (float64 sums of d and d * d), mean and std (population,
    sqrt(max(0, (d_sum2 - d_sum^2 / n) / n)) in float64); mean and std are nan when the region is empty."""
    counts: np.ndarray
    edges: np.ndarray
    below: int
    above: int
    count: int
    d_min: float
    d_max: float
    d_sum: float
    d_sum2: float
    mean: float
    std: float


def otsu_split(counts, edges) -> int:
    """Otsu's split of a histogram, on the host in float64: the k in 0 .. B - 2 that maximises the between-class variance
    w0 w1 (mu0 - mu1)^2 of the classes bins 0 .. k and k + 1 .. B - 1, the bin centres (edges[k] + edges[k + 1]) / 2 standing for
    the bins; ties go to the lowest k; a split that leaves a class empty has variance 0.  -1 with fewer than two non-empty
    bins.  (Running sums in bin order, so that the JS host's loop gives the same bits.)"""
    c = np.asarray(counts, dtype=np.float64)
    if int(np.count_nonzero(c)) < 2:
        return -1
    e = np.asarray(edges, dtype=np.float64)
    cw, cs = np.cumsum(c), np.cumsum(c * ((e[:-1] + e[1:]) / 2))
    w0, s0 = cw[:-1], cs[:-1]
    w1, s1 = cw[-1] - w0, cs[-1] - s0
    ok = (w0 > 0) & (w1 > 0)
    var = np.zeros_like(w0)
    var[ok] = w0[ok] * w1[ok] * (s0[ok] / w0[ok] - s1[ok] / w1[ok]) ** 2
    return int(np.argmax(var))   # (argmax returns the first of equal maxima)


class SegmentMixin:
    def segment(self, seed, lo: float, hi: float = math.inf, connectivity: int = 6, box=None, max_rounds: int = 0):
        """Seeded region growing (vx_segment, DESIGN.md section 2 "Segmentation"): the connected component of
        lo <= d(i) <= hi (both inclusive; d(i) = (volume_density_scale * v(i)) * volume_inv_maj, the isosurfaces' density at
        q = i) inside `box` that holds the voxel `seed` = (x, y, z).  connectivity: 6 (faces) or 26 (faces, edges, corners).
        box = ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices, or None for the whole volume.  hi = inf stands for the
        largest float32.  max_rounds: a cap on the flood's rounds (0: no practical cap); a capped flood returns
        converged = False and a connected part of the segment.  Binds the current uniforms first.  Returns a `Segment`; the
        mask stays on the device (segment_mask, slice_mask) until the next segment or upload."""
        ext = self._index_extent("segment")
        q = _abi.VxSegmentParams()
        q.seed[:] = _checks.voxel("seed", seed, ext)
        q.lo, q.hi = (float(a) for a in _checks.band(lo, hi))
        q.connectivity = _checks.connectivity(connectivity)
        q.box_lo[:], q.box_hi[:] = _checks.box(box, ext)
        q.max_rounds = _checks.integer(max_rounds, 0, 2 ** 32 - 1,
                                       f"max_rounds must be an integer 0 .. 2^32 - 1, not {max_rounds!r}")
        return self._segment_call("vx_segment", C.byref(q))

    def _segment_call(self, fn: str, *args) -> Segment:
        """binds the current uniforms, runs the entry point fn(ctx, *args, &result) and returns the result's `Segment`"""
        p = self.bind_uniforms()
        res = _abi.VxSegmentResult()
        self._check(getattr(self._lib, fn)(self._ctx, *args, C.byref(res)))
        return self._segment_result(res, p)

    def _segment_result(self, res, p, restart: bool = True) -> Segment:
        """the `Segment` of a VxSegmentResult under the uniforms p just bound (segment, segment_edit, set_segment_mask); the
        masked views show the new mask, so accumulation restarts when one is on"""
        if restart and self.segment_view != "off":
            self.restart_rendering()
        g3 = np.asarray(self.volume.grid.transform, dtype=np.float64)[:3, :3]
        d3 = np.asarray(p.density_transform[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T[:3, :3]
        n = int(res.count)
        return Segment(count=n, bbox_lo=tuple(res.bbox_lo[:]), bbox_hi=tuple(res.bbox_hi[:]), d_min=float(res.d_min),
                       d_max=float(res.d_max), d_sum=float(res.d_sum), mean=float(res.d_sum) / n if n else math.nan,
                       rounds=int(res.rounds), converged=bool(res.converged), brick_visits=int(res.brick_visits),
                       volume_grid=n * abs(float(np.linalg.det(g3))), volume_world=n * abs(float(np.linalg.det(d3))))

    SEGMENT_EDIT_OPS = ("dilate", "erode", "open", "close", "fill_holes")   # VxSegmentEditOp, in order

    def segment_edit(self, op: str, steps: int = 1, connectivity: int = 6, band: bool = False) -> Segment:
        """Edits the current segment on the GPU (vx_segment_edit, DESIGN.md section 2 "Segment edits"): "dilate" / "erode" by
        `steps` voxels of the 6- or 26-neighbourhood (outside the volume counts as not set for dilate and as set for erode),
        "open" (erode then dilate), "close" (dilate then erode), or "fill_holes" (the background components, under
        `connectivity`, that touch no face of the volume; steps is ignored).  band=True (dilate only) grows only into voxels
        that pass the predicate of the last segment().  Binds the current uniforms first; returns the `Segment` of the edited
        mask (rounds and brick_visits: the fill's background flood)."""
        self._index_extent("segment_edit")
        if op not in self.SEGMENT_EDIT_OPS:
            raise ValueError(f"op must be one of {self.SEGMENT_EDIT_OPS}, not {op!r}")
        q = _abi.VxSegmentEditParams()
        q.op, q.connectivity = _abi.SEGEDIT_OPS[op], _checks.connectivity(connectivity)
        lo, hi = (0, 1) if op == "fill_holes" else (1, _abi.SEGEDIT_MAX_STEPS)
        q.steps = _checks.integer(steps, lo, hi, f"steps must be an integer {lo} .. {hi} for {op}, not {steps!r}",
                                  whole_floats=False)
        if not isinstance(band, (bool, np.bool_)):
            raise ValueError(f"band must be a bool, not {band!r}")
        if band and op != "dilate":
            raise ValueError(f"band is for dilate only, not {op}")
        q.band = int(bool(band))
        return self._segment_call("vx_segment_edit", C.byref(q))

    MARGIN_OPS = ("grow", "shrink", "open", "close")   # VxMarginOp, in order

    def segment_margin(self, op: str, radius: float, spacing=None, band: bool = False) -> Segment:
        """Edits the current segment by a margin in physical units (vx_segment_margin, DESIGN.md section 2 "Distances and
        margins"): "grow" adds every voxel whose centre lies within `radius` of a voxel centre of the segment, "shrink" removes
        every voxel within `radius` of one outside it (outside the volume counts as inside: a structure cut by the edge of
        the scan does not shrink from there), "close" = grow then shrink, "open" = shrink then grow.  spacing = (s_x, s_y,
        s_z) in the units of radius; None: the column norms of grid.transform (mm for DICOM, the units of volume_grid).
        band=True (grow only) adds only voxels that pass the predicate of the last segment() / threshold().  One exact
        Euclidean transform per half, whatever the radius.  Binds the current uniforms first; returns the `Segment` of the new
        mask."""
        self._index_extent("segment_margin")
        if op not in self.MARGIN_OPS:
            raise ValueError(f"op must be one of {self.MARGIN_OPS}, not {op!r}")
        q = _abi.VxMarginParams()
        q.op, q.radius = _abi.MARGIN_OPS[op], _checks.distance("radius", radius, allow_inf=False)
        q.spacing[:] = _checks.spacing(spacing, self.volume.grid.transform)
        if not isinstance(band, (bool, np.bool_)):
            raise ValueError(f"band must be a bool, not {band!r}")
        if band and op != "grow":
            raise ValueError(f"band is for grow only, not {op}")
        q.band = int(bool(band))
        return self._segment_call("vx_segment_margin", C.byref(q))

    DISTANCE_SIDES = ("outside", "inside")   # VxDistanceSide, in order

    def segment_distance(self, side: str = "outside", max_distance: float = math.inf, spacing=None) -> SegmentDistance:
        """The exact Euclidean distance field of the current segment (vx_segment_distance): side "outside" = how far every
        voxel centre is from the nearest voxel centre of the segment (0 inside it), "inside" = how far every voxel of the segment
        is from the nearest voxel outside it (0 outside; voxels beyond the volume are never candidates).  Distances above
        max_distance read inf.  spacing as for segment_margin.  The segment is not changed.  Returns a `SegmentDistance`."""
        self._index_extent("segment_distance")
        if side not in self.DISTANCE_SIDES:
            raise ValueError(f"side must be one of {self.DISTANCE_SIDES}, not {side!r}")
        q = _abi.VxDistanceParams()
        q.max_distance = _checks.distance("max_distance", max_distance, allow_inf=True)
        q.spacing[:] = _checks.spacing(spacing, self.volume.grid.transform)
        q.side = _abi.DISTANCE_SIDES[side]
        self.bind_uniforms()
        res = _abi.VxDistanceResult()
        self._check(self._lib.vx_segment_distance(self._ctx, C.byref(q), C.byref(res)))
        return SegmentDistance(self, res, side, tuple(q.spacing[:]), float(q.max_distance))

    def distance_field(self) -> np.ndarray:
        """the squared distances of the last segment_distance as a (Z, Y, X) float32 array, inf beyond the cap
        (vx_distance_read); refused once the segment has changed"""
        X, Y, Z = self._index_extent("distance_field", hint="")
        out = np.empty((Z, Y, X), dtype=np.float32)
        self._check(self._lib.vx_distance_read(self._ctx, out.ctypes.data, out.size))
        return out

    def distance_stats(self):
        """(launches, x_ms, y_ms, z_ms, compare_ms) of the last segment_distance or segment_margin (vx_distance_stats); the
        passes of open / close are summed over their two transforms"""
        return self._out("vx_distance_stats", C.c_uint32, C.c_double * 4)

    def set_segment_mask(self, mask) -> Segment:
        """Installs a (Z, Y, X) bool array over the index extent as the current segment (vx_segment_write_mask, the inverse of
        segment_mask): a saved segmentation or a mask made on the host (combinations and undo have a GPU path: store_segment,
        segment_combine).  The predicate of the last
        segment() and the segment view stay.  Binds the current uniforms first; returns the mask's `Segment`."""
        X, Y, Z = self._index_extent("set_segment_mask")
        m = np.asarray(mask)
        if m.dtype != np.bool_:
            raise ValueError(f"mask must be a bool array, not {m.dtype}")
        if m.shape != (Z, Y, X):
            raise ValueError(f"mask shape must be (Z, Y, X) = {(Z, Y, X)} of the index extent, not {m.shape}")
        bits = np.packbits(np.ascontiguousarray(m).ravel(), bitorder="little")
        return self._segment_call("vx_segment_write_mask", bits.ctypes.data, bits.size)

    def segment_edit_stats(self):
        """(launches, edit_ms, stats_ms) of the last segment_edit or set_segment_mask (vx_segment_edit_stats)"""
        return self._out("vx_segment_edit_stats", C.c_uint32, C.c_double * 2)

    def threshold(self, lo: float, hi: float = math.inf, box=None) -> Segment:
        """The whole band as the current segment, without a seed (vx_segment_threshold): every voxel with lo <= d(i) <= hi
        inside `box`; arguments as for segment().  It also becomes the predicate of band dilation.  Returns its `Segment`
        (rounds = brick_visits = 0)."""
        ext = self._index_extent("threshold")
        q = _abi.VxSegmentParams()
        q.lo, q.hi = (float(a) for a in _checks.band(lo, hi))
        q.connectivity = 6
        q.box_lo[:], q.box_hi[:] = _checks.box(box, ext)
        return self._segment_call("vx_segment_threshold", C.byref(q))

    def _islands_call(self, name, op, connectivity, keep=0, min_voxels=0, seed=(0, 0, 0)):
        self._index_extent(name)
        q = _abi.VxIslandsParams()
        q.op, q.connectivity, q.keep, q.min_voxels = _abi.ISLANDS_OPS[op], _checks.connectivity(connectivity), keep, min_voxels
        q.seed[:] = seed
        p = self.bind_uniforms()
        res = _abi.VxIslandsResult()
        self._check(self._lib.vx_segment_islands(self._ctx, C.byref(q), C.byref(res)))
        self._island_rows = int(res.kept)
        # (labelling leaves the mask as it was: a masked view does not restart)
        return res, self._segment_result(res.seg, p, restart=op != "label")

    def _island_segment(self, res, seg) -> IslandSegment:
        return IslandSegment(**{f: getattr(seg, f) for f in Segment.__dataclass_fields__}, islands=int(res.islands),
                             kept=int(res.kept), largest=int(res.largest))

    def islands(self, connectivity: int = 6) -> Islands:
        """Labels the islands of the current segment on the GPU (vx_segment_islands, DESIGN.md section 2 "Islands"): its 6- or
        26-connected components, ordered by voxel count descending, ties by the first voxel in C order.  The segment is not
        changed.  Returns an `Islands` (count, sizes, table, labels())."""
        res, seg = self._islands_call("islands", "label", connectivity)
        return Islands(self, res, self.island_table(), seg)

    def island_table(self, first: int = 0, n: int | None = None):
        """rows first .. first + n - 1 (default: all the rest) of the current island table as VxIsland structs (vx_islands_read)"""
        if n is None:
            n = max(getattr(self, "_island_rows", 0) - int(first), 0)
        rows = (_abi.VxIsland * max(int(n), 1))()
        self._check(self._lib.vx_islands_read(self._ctx, int(first), int(n), rows))
        return list(rows[:int(n)])

    def island_labels(self) -> np.ndarray:
        """the dense (Z, Y, X) uint32 label volume of the current island table: 0 outside the segment, k + 1 for island k
        (vx_islands_read_labels)"""
        X, Y, Z = self._index_extent("island_labels", hint="")
        out = np.empty((Z, Y, X), dtype=np.uint32)
        self._check(self._lib.vx_islands_read_labels(self._ctx, out.ctypes.data, out.size))
        return out

    def keep_largest_islands(self, n: int = 1, connectivity: int = 6) -> IslandSegment:
        """Keeps the n largest islands of the current segment (canonical order; n >= the number of islands keeps all).  Returns
        the `Segment` of the new mask with .islands (before), .kept (after) and .largest."""
        n = _checks.integer(n, 1, 2 ** 64 - 1, f"n must be an integer >= 1, not {n!r}", whole_floats=False)
        return self._island_segment(*self._islands_call("keep_largest_islands", "keep_largest", connectivity, keep=n))

    def remove_small_islands(self, min_voxels: int, connectivity: int = 6) -> IslandSegment:
        """Removes the islands of fewer than min_voxels voxels from the current segment (none left is legal)."""
        min_voxels = _checks.integer(min_voxels, 1, 2 ** 64 - 1, f"min_voxels must be an integer >= 1, not {min_voxels!r}",
                                     whole_floats=False)
        return self._island_segment(*self._islands_call("remove_small_islands", "remove_small", connectivity,
                                                        min_voxels=min_voxels))

    def keep_island_at(self, voxel, connectivity: int = 6) -> IslandSegment:
        """Keeps the island of the current segment that holds `voxel` = (x, y, z); the empty set when the voxel is not in it."""
        sd = _checks.voxel("voxel", voxel, self._index_extent("keep_island_at"))
        return self._island_segment(*self._islands_call("keep_island_at", "keep_at", connectivity, seed=sd))

    def islands_stats(self):
        """(launches, local_ms, merge_ms, flatten_ms, table_ms, host_rank_ms, apply_ms, stats_ms) of the last islands call
        (vx_islands_stats); host_rank_ms is the host's wall clock for reading back, ranking and re-uploading the rows"""
        return self._out("vx_islands_stats", C.c_uint32, C.c_double * 7)

    # ---- the segment store (DESIGN.md section 2 "Segment store") ----------------------------------------------------------------
    COMBINE_OPS = ("union", "intersect", "subtract", "xor", "invert")   # VxCombineOp, in order

    def store_segment(self, slot: int) -> None:
        """Copies the current segment into `slot` (0 .. 31) of the device's segment store, replacing what it held
        (vx_segment_store); the current segment stays.  A slot costs 1 bit per voxel and lasts until drop_segment or the next
        setup_from_grid."""
        self._index_extent("store_segment")
        slot = _checks.slot(slot)
        self.bind_uniforms()
        self._check(self._lib.vx_segment_store(self._ctx, slot))

    def load_segment(self, slot: int) -> Segment:
        """Makes the mask of `slot` the current segment (vx_segment_load): an undo, or the start of the next edit.  The slot
        keeps its copy; the predicate of the last segment() / threshold() stays.  Returns the mask's `Segment`."""
        self._index_extent("load_segment")
        return self._segment_call("vx_segment_load", _checks.slot(slot))

    def drop_segment(self, slot: int) -> None:
        """frees `slot` (vx_segment_drop); an empty slot is fine"""
        self._index_extent("drop_segment")
        slot = _checks.slot(slot)
        self.bind_uniforms()
        self._check(self._lib.vx_segment_drop(self._ctx, slot))

    def stored_segments(self) -> tuple:
        """the occupied slots, ascending (vx_segment_slots)"""
        self._index_extent("stored_segments")
        self.bind_uniforms()
        bits = self._out("vx_segment_slots", C.c_uint32)[0]
        return tuple(k for k in range(_abi.SEGMENT_SLOTS) if bits >> k & 1)

    def segment_combine(self, op: str, slot: int | None = None) -> Segment:
        """A set operation on the current segment A and the mask B of `slot`, in place on the GPU (vx_segment_combine): "union"
        A | B, "intersect" A & B, "subtract" A & ~B, "xor" A ^ B, or "invert" ~A over the index extent (padding included), which
        takes no slot.  The slot is not changed.  Binds the current uniforms first; returns the `Segment` of the new mask."""
        self._index_extent("segment_combine")
        if op not in self.COMBINE_OPS:
            raise ValueError(f"op must be one of {self.COMBINE_OPS}, not {op!r}")
        if (op == "invert") != (slot is None):
            raise ValueError("slot must be None for invert" if op == "invert" else f"slot is required for {op}")
        q = _abi.VxCombineParams()
        q.op, q.slot = _abi.COMBINE_OPS[op], 0 if slot is None else _checks.slot(slot)
        return self._segment_call("vx_segment_combine", C.byref(q))

    def segment_compare(self, slot: int, hausdorff: bool = True, spacing=None) -> SegmentComparison:
        """Compares the current segment A with the mask B of `slot` (vx_segment_compare): the exact overlap counts with Dice and
        Jaccard, and with hausdorff=True the two directed Hausdorff distances from two exact Euclidean transforms (spacing as
        for segment_margin).  Neither mask is changed; with hausdorff=True the field of the last segment_distance is
        overwritten.  Returns a `SegmentComparison`."""
        self._index_extent("segment_compare")
        q = _abi.VxCompareParams()
        q.slot = _checks.slot(slot)
        if not isinstance(hausdorff, (bool, np.bool_)):
            raise ValueError(f"hausdorff must be a bool, not {hausdorff!r}")
        q.hausdorff = int(bool(hausdorff))
        q.spacing[:] = _checks.spacing(spacing, self.volume.grid.transform)
        self.bind_uniforms()
        res = _abi.VxCompareResult()
        self._check(self._lib.vx_segment_compare(self._ctx, C.byref(q), C.byref(res)))
        a, b, n = int(res.count_a), int(res.count_b), int(res.count_and)
        kw = dict(count_a=a, count_b=b, count_and=n, dice=2 * n / (a + b) if a + b else math.nan,
                  jaccard=n / (a + b - n) if a + b else math.nan)
        if hausdorff:
            ab, ba = (float(np.sqrt(np.float32(v))) for v in (res.d2_ab, res.d2_ba))
            kw.update(d2_ab=float(res.d2_ab), d2_ba=float(res.d2_ba), hausdorff_ab=ab, hausdorff_ba=ba, hausdorff=max(ab, ba),
                      argmax_ab=tuple(res.argmax_ab[:]), argmax_ba=tuple(res.argmax_ba[:]))
        return SegmentComparison(**kw)

    def segments_labelmap(self, slots):
        """The label map of the listed slots (vx_segments_labelmap): a (Z, Y, X) uint8 array with k + 1 where slots[k] is the
        first listed slot that holds the voxel and 0 where none does, and the number of voxels more than one listed slot
        holds.  Returns (labels, overlaps): how a multi-segment segmentation is saved."""
        X, Y, Z = self._index_extent("segments_labelmap")
        t = _checks.slots(slots)
        self.bind_uniforms()
        out = np.empty((Z, Y, X), dtype=np.uint8)
        over = C.c_uint64()
        self._check(self._lib.vx_segments_labelmap(self._ctx, (C.c_uint32 * len(t))(*t), len(t), out.ctypes.data, out.size,
                                                   C.byref(over)))
        return out, int(over.value)

    # ---- histograms (DESIGN.md section 2 "Histograms") --------------------------------------------------------------------------
    def _histogram_params(self, name: str, source, box):
        ext = self._index_extent(name)
        q = _abi.VxHistogramParams()
        q.source, q.slot = _checks.hist_source(source)
        q.box_lo[:], q.box_hi[:] = _checks.box(box, ext)
        return q

    def _histogram_call(self, q, nbins: int):
        """vx_histogram under the uniforms already bound: (counts, VxHistogramResult)"""
        counts = np.zeros(nbins, dtype=np.uint64)
        res = _abi.VxHistogramResult()
        self._check(self._lib.vx_histogram(self._ctx, C.byref(q), counts.ctypes.data, nbins, C.byref(res)))
        return counts, res

    def histogram(self, bins: int = 256, range=(0.0, 1.0), source="volume", box=None) -> Histogram:
        """The density histogram and the moments of a region on the GPU (vx_histogram, DESIGN.md section 2 "Histograms").
        source: "volume" (every voxel), "segment" (the current segment) or an int (that slot of the segment store); box =
        ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices, or None for the whole index extent (padding included).  `bins`
        bins of equal width over range = (lo, hi), the span the transfer function covers by default; a density equal to hi
        lands in the last bin, as in np.histogram.  Binds the current uniforms first; changes nothing.  Returns a `Histogram`."""
        q = self._histogram_params("histogram", source, box)
        q.rule, q.bins = _abi.HIST_LINEAR, _checks.hist_bins(bins)
        q.lo, q.hi = _checks.hist_range(range)
        q.moments = 1
        self.bind_uniforms()
        counts, res = self._histogram_call(q, q.bins)
        n, s1, s2 = int(res.count), float(res.d_sum), float(res.d_sum2)
        lo, hi = float(q.lo), float(q.hi)
        edges = lo + np.arange(q.bins + 1, dtype=np.float64) * (hi - lo) / q.bins
        return Histogram(counts=counts, edges=edges, below=int(res.below), above=int(res.above), count=n, d_min=float(res.d_min),
                         d_max=float(res.d_max), d_sum=s1, d_sum2=s2, mean=s1 / n if n else math.nan,
                         std=math.sqrt(max(0.0, (s2 - s1 * s1 / n) / n)) if n else math.nan)

    RADIX_PASSES = ((0, 11), (11, 11), (22, 10))   # (prefix_bits, key_bits) of the three passes of the select

    def _order_statistics(self, q, ranks_of):
        """the radix select behind density_order_statistic and density_percentile: ranks_of(n) -> the ranks, given the size of
        the region from the first pass, which all ranks share (as they share every later pass with the same prefix)"""
        q.rule, q.moments = _abi.HIST_KEY, 0
        self.bind_uniforms()
        seen = {}

        def counts_of(p, b, prefix):
            if (p, prefix) not in seen:
                q.prefix, q.prefix_bits, q.key_bits = prefix, p, b
                seen[(p, prefix)] = self._histogram_call(q, 1 << b)
            return seen[(p, prefix)]

        n = int(counts_of(*self.RADIX_PASSES[0], 0)[1].count)
        out = []
        for k in ranks_of(n):
            prefix = 0
            for p, b in self.RADIX_PASSES:
                # `below` holds every key under a smaller prefix: rank k of the region is rank k - below among this pass's bins
                c, res = counts_of(p, b, prefix)
                j = int(np.searchsorted(np.cumsum(c.astype(np.int64)), k - int(res.below), side="right"))
                prefix = (prefix << b) | j
            key = prefix
            u = key & 0x7fffffff if key & 0x80000000 else ~key & 0xffffffff
            out.append(np.array([u], dtype=np.uint32).view(np.float32)[0])
        return np.array(out, dtype=np.float32), n

    def density_order_statistic(self, ranks, source="volume", box=None) -> np.ndarray:
        """The exact k-th smallest densities (0-based ranks) of a region, as float32: the bits of np.sort(d[R])[k].  A radix
        select over the order-preserving key of the densities in three histogram passes (11, 11 and 10 bits) per rank; the
        first pass is shared by all ranks.  source and box as for histogram().  An empty region is refused."""
        q = self._histogram_params("density_order_statistic", source, box)
        _checks.ranks(ranks)

        def ranks_of(n):
            if n == 0:
                raise VolxelError("density_order_statistic: the region is empty")
            return _checks.ranks(ranks, n)
        return self._order_statistics(q, ranks_of)[0]

    def density_percentile(self, q, source="volume", box=None):
        """The q-th percentile(s) of the densities of a region, exact: the order statistic of rank floor(q / 100 * (n - 1))
        computed in float64 -- np.percentile(d[R], q, method="lower").  q: a number (returns a float) or a sequence of numbers
        (returns a float32 array) in [0, 100].  source and box as for histogram().  An empty region is refused."""
        qs, scalar = _checks.percentiles(q)
        hp = self._histogram_params("density_percentile", source, box)

        def ranks_of(n):
            if n == 0:
                raise VolxelError("density_percentile: the region is empty")
            return [int(math.floor(a / 100.0 * (n - 1))) for a in qs]
        v = self._order_statistics(hp, ranks_of)[0]
        return float(v[0]) if scalar else v

    def otsu_threshold(self, bins: int = 256, range=(0.0, 1.0), source="volume", box=None) -> float:
        """Otsu's threshold of a region from one histogram() of `bins` bins over `range`: the upper edge of the bin k that
        maximises the between-class variance (otsu_split), so that threshold(t) is the bright class.  Voxels below or above
        the range are ignored.  Fewer than two non-empty bins are refused."""
        h = self.histogram(bins, range, source, box)
        k = otsu_split(h.counts, h.edges)
        if k < 0:
            raise VolxelError(f"otsu_threshold: fewer than two non-empty bins among the {h.counts.size} over {tuple(range)!r}: "
                             "nothing to split")
        return float(h.edges[k + 1])

    def histogram_stats(self):
        """(launches, histogram_ms, moments_ms) of the last histogram pass (vx_histogram_stats)"""
        return self._out("vx_histogram_stats", C.c_uint32, C.c_double * 2)

    SEGMENT_VIEWS = ("off", "only", "hide")   # VX_SEGVIEW_OFF, _ONLY, _HIDE

    @property
    def segment_view(self) -> str:
        """"off" (the default, and again after setup_from_grid), "only" (the current segment alone) or "hide" (everything but
        it): DVR, Phong, MIP / MinIP renders and the isosurfaces (hence pick) sample a volume whose hidden voxels read 0
        (vx_set_segment_view, DESIGN.md section 2 "Segment views"); slices and segment() keep the unmasked data"""
        return self.SEGMENT_VIEWS[self._out("vx_get_segment_view", C.c_int32)[0]]

    @segment_view.setter
    def segment_view(self, view: str):
        if view not in self.SEGMENT_VIEWS:
            raise VolxelError(f"segment_view must be one of {self.SEGMENT_VIEWS}, not {view!r}")
        self._check(self._lib.vx_set_segment_view(self._ctx, self.SEGMENT_VIEWS.index(view)))
        self.restart_rendering()

    def segment_mask(self) -> np.ndarray:
        """the current segment as a (Z, Y, X) bool array over the index extent (vx_segment_read_mask)"""
        X, Y, Z = self._index_extent("segment_mask", hint="")
        bits = np.empty(X * Y * Z // 8, dtype=np.uint8)
        self._check(self._lib.vx_segment_read_mask(self._ctx, bits.ctypes.data, bits.size))
        return np.unpackbits(bits, bitorder="little").astype(bool).reshape(Z, Y, X)

    def slice_mask(self, sp) -> np.ndarray:
        """the current segment on the slice or slab sp (volxel_amd.mpr; reduce, display and window are ignored): an (H, W)
        bool array, True where the nearest voxel of any slab sample is in the segment (vx_slice_segment_mask)"""
        if not isinstance(sp, _abi.VxSliceParams):
            raise TypeError("sp must be a VxSliceParams (volxel_amd.mpr builds them)")
        W, H, _ = _checks.slice_spec(sp)
        out = np.empty((H, W), dtype=np.uint8)
        self._check(self._lib.vx_slice_segment_mask(self._ctx, C.byref(sp), out.ctypes.data))
        return out.astype(bool)

    def segment_stats(self):
        """(rounds, brick_visits, predicate_ms, flood_ms, stats_ms) of the last segment; flood_ms runs from the first round to
        the last, the host's read-backs of the worklist length included"""
        return self._out("vx_segment_stats", C.c_uint32, C.c_uint64, C.c_double * 3)

    def voxel_index(self, world_point):
        """the voxel (x, y, z) nearest a world point, or None outside the volume: q = density_transform_inv * w - 1/2 in float64
        (the current params, as mpr.oblique maps planes), then floor(q + 1/2) per axis.  A point from pick() lies on the
        interpolated surface, so its nearest voxel can fall just below the threshold: seed a segment with it where the
        structure is thicker than a voxel, or lower lo a little."""
        ext = self._index_extent("voxel_index", hint="")
        w = np.asarray(world_point, dtype=np.float64).reshape(-1)
        if w.size != 3 or not np.isfinite(w).all():
            raise ValueError(f"world_point must be three finite numbers, not {world_point!r}")
        # the float32 matrix the uniforms carry now (compute_params, as bind_uniforms sends it), not a copy from an earlier bind
        from .renderer import compute_params
        p = compute_params(self.settings, self.camera, self.volume, self.density_scale, self.width, self.height,
                           self.env_strength, self.shard_rank, self.shard_count, has_environment=self.environment is not None)
        m = [float(v) for v in np.asarray(p.density_transform_inv[:], dtype=np.float32)]   # column major
        # q = m * w - 1/2 in float64, each row summed x, y, z, translation in that order (the JS host's voxelIndex sums alike)
        qv = [m[r] * w[0] + m[4 + r] * w[1] + m[8 + r] * w[2] + m[12 + r] - 0.5 for r in range(3)]
        i = [math.floor(a + 0.5) for a in qv]
        if not all(0 <= a < e for a, e in zip(i, ext)):
            return None
        return tuple(int(a) for a in i)
