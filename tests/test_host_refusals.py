"""The refusals of the two host layers, pinned word for word (no device: every call here is refused, or arrives at the
uniforms, before the library is reached).

The Python host (volxel_amd.Volxel3DRenderer) and the JavaScript host (napi/viewer.js) check their arguments before they bind
the uniforms.  Each table below holds a call, the exception type and the exact message: one case per check and per method that
makes it, so that the checks several methods share (box, band, voxel, connectivity, slice spec) stay the same text in each of
them; the texts without a volume; calls with two faults, where the first check's message wins; and calls that pass every check
(they arrive at bind_uniforms / bindUniforms, which a marker replaces), which pins what the checks let through: whole floats
pass the checks written int(x) != x and not those written isinstance(x, int)."""
import json
import shutil
import subprocess
import types

import numpy as np
import pytest

from tests.common import NAPI
from tests.shapes import ISO_PHONG, renderer_shell
from volxel_amd import VolxelError, mpr

nan, inf = float("nan"), float("inf")


class Bound(Exception):
    """raised in place of bind_uniforms: every check before it has passed"""


def shell(kind="vol"):
    """a renderer without a context: "vol" has the (16, 16, 24) volume description, "none" has no volume, "bound" raises
    Bound where it would bind the uniforms"""
    r = renderer_shell()
    r.settings = types.SimpleNamespace(phong=ISO_PHONG)
    r.width, r.height = 32, 24
    if kind == "none":
        r.volume = None
    if kind == "bound":
        def bound():
            raise Bound("bind_uniforms")
        r.bind_uniforms = bound
    return r


def sp(**fields):
    """the axial plane k = 3 of the shell's volume with some fields replaced"""
    q = mpr.axial(renderer_shell(), 3)
    for k, v in fields.items():
        if k == "slab_samples":
            q.slab_samples = v
        else:
            getattr(q, k)[:] = v
    return q


# ---- the tables: (id, call, exception type, message) -----------------------------------------------------------------
PY = [
    ("segment/seed-two", lambda r: r.segment((0, 0), 0.1),
     ValueError, "seed must be three integer voxel indices (x, y, z), not (0, 0)"),
    ("segment/seed-float", lambda r: r.segment((0.5, 0, 0), 0.1),
     ValueError, "seed must be three integer voxel indices (x, y, z), not (0.5, 0, 0)"),
    ("segment/seed-bool", lambda r: r.segment((True, 0, 0), 0.1),
     ValueError, "seed must be three integer voxel indices (x, y, z), not (True, 0, 0)"),
    ("segment/seed-x-outside", lambda r: r.segment((16, 0, 0), 0.1),
     ValueError, "seed (16, 0, 0) is outside the index extent (16, 16, 24)"),
    ("segment/seed-negative", lambda r: r.segment((0, 0, -1), 0.1),
     ValueError, "seed (0, 0, -1) is outside the index extent (16, 16, 24)"),
    ("segment/lo-nan", lambda r: r.segment((1, 1, 1), nan),
     ValueError, "lo and hi must be finite (hi may be inf), not nan, inf"),
    ("segment/hi-nan", lambda r: r.segment((1, 1, 1), 0.1, nan),
     ValueError, "lo and hi must be finite (hi may be inf), not 0.1, nan"),
    ("segment/lo-minus-inf", lambda r: r.segment((1, 1, 1), -inf),
     ValueError, "lo and hi must be finite (hi may be inf), not -inf, inf"),
    ("segment/lo-above-hi", lambda r: r.segment((1, 1, 1), 0.5, 0.4),
     ValueError, "lo = 0.5 > hi = 0.4"),
    ("segment/connectivity-18", lambda r: r.segment((1, 1, 1), 0.1, connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("segment/connectivity-bool", lambda r: r.segment((1, 1, 1), 0.1, connectivity=True),
     ValueError, "connectivity must be 6 or 26, not True"),
    ("segment/box-not-a-pair", lambda r: r.segment((1, 1, 1), 0.1, box=(1, 2)),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)), not (1, 2)"),
    ("segment/box-one-corner", lambda r: r.segment((1, 1, 1), 0.1, box=((0, 0, 0),)),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)), not ((0, 0, 0),)"),
    ("segment/box-short-corner", lambda r: r.segment((1, 1, 1), 0.1, box=((0, 0), (1, 1, 1))),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not ((0, 0), (1, 1, 1))"),
    ("segment/box-float", lambda r: r.segment((1, 1, 1), 0.1, box=((0, 0, 0), (1.5, 2, 2))),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not ((0, 0, 0), (1.5, 2, 2))"),
    ("segment/box-empty", lambda r: r.segment((1, 1, 1), 0.1, box=((2, 0, 0), (1, 5, 5))),
     ValueError, "box ((2, 0, 0), (1, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("segment/box-outside", lambda r: r.segment((1, 1, 1), 0.1, box=((0, 0, 0), (16, 5, 5))),
     ValueError, "box ((0, 0, 0), (16, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("segment/max-rounds-negative", lambda r: r.segment((1, 1, 1), 0.1, max_rounds=-1),
     ValueError, "max_rounds must be an integer 0 .. 2^32 - 1, not -1"),
    ("segment/max-rounds-2^32", lambda r: r.segment((1, 1, 1), 0.1, max_rounds=2 ** 32),
     ValueError, "max_rounds must be an integer 0 .. 2^32 - 1, not 4294967296"),
    ("segment/max-rounds-float", lambda r: r.segment((1, 1, 1), 0.1, max_rounds=1.5),
     ValueError, "max_rounds must be an integer 0 .. 2^32 - 1, not 1.5"),
    ("segment/max-rounds-bool", lambda r: r.segment((1, 1, 1), 0.1, max_rounds=True),
     ValueError, "max_rounds must be an integer 0 .. 2^32 - 1, not True"),
    ("threshold/lo-nan", lambda r: r.threshold(nan),
     ValueError, "lo and hi must be finite (hi may be inf), not nan, inf"),
    ("threshold/hi-minus-inf", lambda r: r.threshold(0.1, -inf),
     ValueError, "lo and hi must be finite (hi may be inf), not 0.1, -inf"),
    ("threshold/lo-above-hi", lambda r: r.threshold(0.5, 0.4),
     ValueError, "lo = 0.5 > hi = 0.4"),
    ("threshold/box-not-a-pair", lambda r: r.threshold(0.1, box=(1, 2)),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)), not (1, 2)"),
    ("threshold/box-float", lambda r: r.threshold(0.1, box=((0, 0, 0), (1.5, 2, 2))),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not ((0, 0, 0), (1.5, 2, 2))"),
    ("threshold/box-empty", lambda r: r.threshold(0.1, box=((2, 0, 0), (1, 5, 5))),
     ValueError, "box ((2, 0, 0), (1, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("threshold/box-outside", lambda r: r.threshold(0.1, box=((0, 0, 0), (0, 0, 24))),
     ValueError, "box ((0, 0, 0), (0, 0, 24)) is empty or outside the index extent (16, 16, 24)"),
    ("segment_edit/op-unknown", lambda r: r.segment_edit('grow'),
     ValueError, "op must be one of ('dilate', 'erode', 'open', 'close', 'fill_holes'), not 'grow'"),
    ("segment_edit/op-int", lambda r: r.segment_edit(0),
     ValueError, "op must be one of ('dilate', 'erode', 'open', 'close', 'fill_holes'), not 0"),
    ("segment_edit/connectivity-18", lambda r: r.segment_edit('dilate', connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("segment_edit/connectivity-bool", lambda r: r.segment_edit('dilate', connectivity=True),
     ValueError, "connectivity must be 6 or 26, not True"),
    ("segment_edit/steps-0", lambda r: r.segment_edit('dilate', steps=0),
     ValueError, "steps must be an integer 1 .. 1024 for dilate, not 0"),
    ("segment_edit/steps-1025", lambda r: r.segment_edit('erode', steps=1025),
     ValueError, "steps must be an integer 1 .. 1024 for erode, not 1025"),
    ("segment_edit/steps-1.5", lambda r: r.segment_edit('open', steps=1.5),
     ValueError, "steps must be an integer 1 .. 1024 for open, not 1.5"),
    ("segment_edit/steps-1.0", lambda r: r.segment_edit('dilate', steps=1.0),
     ValueError, "steps must be an integer 1 .. 1024 for dilate, not 1.0"),
    ("segment_edit/steps-bool", lambda r: r.segment_edit('close', steps=True),
     ValueError, "steps must be an integer 1 .. 1024 for close, not True"),
    ("segment_edit/fill-steps-2", lambda r: r.segment_edit('fill_holes', steps=2),
     ValueError, "steps must be an integer 0 .. 1 for fill_holes, not 2"),
    ("segment_edit/band-int", lambda r: r.segment_edit('dilate', band=1),
     ValueError, "band must be a bool, not 1"),
    ("segment_edit/band-erode", lambda r: r.segment_edit('erode', band=True),
     ValueError, "band is for dilate only, not erode"),
    ("segment_edit/band-fill", lambda r: r.segment_edit('fill_holes', band=True),
     ValueError, "band is for dilate only, not fill_holes"),
    ("set_segment_mask/uint8", lambda r: r.set_segment_mask(np.zeros((24, 16, 16), dtype=np.uint8)),
     ValueError, "mask must be a bool array, not uint8"),
    ("set_segment_mask/xyz-order", lambda r: r.set_segment_mask(np.zeros((16, 16, 24), dtype=bool)),
     ValueError, "mask shape must be (Z, Y, X) = (24, 16, 16) of the index extent, not (16, 16, 24)"),
    ("set_segment_mask/flat", lambda r: r.set_segment_mask(np.zeros(24 * 16 * 16, dtype=bool)),
     ValueError, "mask shape must be (Z, Y, X) = (24, 16, 16) of the index extent, not (6144,)"),
    ("keep_largest_islands/n-0", lambda r: r.keep_largest_islands(0),
     ValueError, "n must be an integer >= 1, not 0"),
    ("keep_largest_islands/n-1.0", lambda r: r.keep_largest_islands(1.0),
     ValueError, "n must be an integer >= 1, not 1.0"),
    ("keep_largest_islands/n-bool", lambda r: r.keep_largest_islands(True),
     ValueError, "n must be an integer >= 1, not True"),
    ("keep_largest_islands/n-2^64", lambda r: r.keep_largest_islands(2 ** 64),
     ValueError, "n must be an integer >= 1, not 18446744073709551616"),
    ("keep_largest_islands/connectivity-18", lambda r: r.keep_largest_islands(2, connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("keep_largest_islands/connectivity-bool", lambda r: r.keep_largest_islands(2, connectivity=True),
     ValueError, "connectivity must be 6 or 26, not True"),
    ("remove_small_islands/min-0", lambda r: r.remove_small_islands(0),
     ValueError, "min_voxels must be an integer >= 1, not 0"),
    ("remove_small_islands/min-2.5", lambda r: r.remove_small_islands(2.5),
     ValueError, "min_voxels must be an integer >= 1, not 2.5"),
    ("remove_small_islands/min-bool", lambda r: r.remove_small_islands(True),
     ValueError, "min_voxels must be an integer >= 1, not True"),
    ("remove_small_islands/connectivity-18", lambda r: r.remove_small_islands(4, connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("keep_island_at/voxel-two", lambda r: r.keep_island_at((0, 0)),
     ValueError, "voxel must be three integer voxel indices (x, y, z), not (0, 0)"),
    ("keep_island_at/voxel-float", lambda r: r.keep_island_at((0.5, 0, 0)),
     ValueError, "voxel must be three integer voxel indices (x, y, z), not (0.5, 0, 0)"),
    ("keep_island_at/voxel-bool", lambda r: r.keep_island_at((True, 0, 0)),
     ValueError, "voxel must be three integer voxel indices (x, y, z), not (True, 0, 0)"),
    ("keep_island_at/voxel-x-outside", lambda r: r.keep_island_at((16, 0, 0)),
     ValueError, "voxel (16, 0, 0) is outside the index extent (16, 16, 24)"),
    ("keep_island_at/voxel-negative", lambda r: r.keep_island_at((0, 0, -1)),
     ValueError, "voxel (0, 0, -1) is outside the index extent (16, 16, 24)"),
    ("keep_island_at/connectivity-18", lambda r: r.keep_island_at((1, 1, 1), connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("keep_island_at/connectivity-bool", lambda r: r.keep_island_at((1, 1, 1), connectivity=True),
     ValueError, "connectivity must be 6 or 26, not True"),
    ("islands/connectivity-18", lambda r: r.islands(18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("islands/connectivity-bool", lambda r: r.islands(connectivity=True),
     ValueError, "connectivity must be 6 or 26, not True"),
    ("extract_mesh/segment-int", lambda r: r.extract_mesh(segment=1),
     ValueError, "segment must be True or False, not 1"),
    ("extract_mesh/neither", lambda r: r.extract_mesh(),
     ValueError, "extract_mesh takes exactly one of iso and segment=True"),
    ("extract_mesh/both", lambda r: r.extract_mesh(0.5, segment=True),
     ValueError, "extract_mesh takes exactly one of iso and segment=True"),
    ("extract_mesh/space", lambda r: r.extract_mesh(0.5, space='mm'),
     ValueError, "space must be one of ('voxel', 'grid', 'world'), not 'mm'"),
    ("extract_mesh/max-vertices-negative", lambda r: r.extract_mesh(0.5, max_vertices=-1),
     ValueError, "max_vertices must be an integer 0 .. 2^32 - 1, not -1"),
    ("extract_mesh/max-vertices-float", lambda r: r.extract_mesh(0.5, max_vertices=1.5),
     ValueError, "max_vertices must be an integer 0 .. 2^32 - 1, not 1.5"),
    ("extract_mesh/max-triangles-2^32", lambda r: r.extract_mesh(0.5, max_triangles=2 ** 32),
     ValueError, "max_triangles must be an integer 0 .. 2^32 - 1, not 4294967296"),
    ("extract_mesh/max-triangles-bool", lambda r: r.extract_mesh(segment=True, max_triangles=True),
     ValueError, "max_triangles must be an integer 0 .. 2^32 - 1, not True"),
    ("extract_mesh/iso-nan", lambda r: r.extract_mesh(nan),
     ValueError, "iso must be finite and > 0, not nan"),
    ("extract_mesh/iso-zero", lambda r: r.extract_mesh(0.0),
     ValueError, "iso must be finite and > 0, not 0.0"),
    ("extract_mesh/iso-negative", lambda r: r.extract_mesh(-1.0),
     ValueError, "iso must be finite and > 0, not -1.0"),
    ("extract_mesh/iso-overflows-float32", lambda r: r.extract_mesh(1e39),
     ValueError, "iso must be finite and > 0, not 1e+39"),
    ("extract_mesh/box-not-a-pair", lambda r: r.extract_mesh(0.5, box=(1, 2)),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)), not (1, 2)"),
    ("extract_mesh/box-float", lambda r: r.extract_mesh(0.5, box=((0, 0, 0), (1.5, 2, 2))),
     ValueError, "box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not ((0, 0, 0), (1.5, 2, 2))"),
    ("extract_mesh/box-empty", lambda r: r.extract_mesh(segment=True, box=((2, 0, 0), (1, 5, 5))),
     ValueError, "box ((2, 0, 0), (1, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("extract_mesh/box-outside", lambda r: r.extract_mesh(0.5, box=((0, 0, 0), (16, 5, 5))),
     ValueError, "box ((0, 0, 0), (16, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("slice/not-a-spec", lambda r: r.slice('axial'),
     TypeError, "sp must be a VxSliceParams (volxel_amd.mpr builds them)"),
    ("slice/reduce", lambda r: r.slice(sp(), reduce='sum'),
     ValueError, "reduce must be one of ['max', 'mean', 'min'], not 'sum'"),
    ("slice/display", lambda r: r.slice(sp(), display='rgb'),
     ValueError, "display must be None, 'grey' or 'tf', not 'rgb'"),
    ("slice/size-0", lambda r: r.slice(sp(size=(0, 16))),
     ValueError, "slice size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice/size-16385", lambda r: r.slice(sp(size=(16, 16385))),
     ValueError, "slice size must be 1 .. 16384 per side, not 16 x 16385"),
    ("slice/slab-0", lambda r: r.slice(sp(slab_samples=0)),
     ValueError, "slab_samples must be 1 .. 4096, not 0"),
    ("slice/slab-4097", lambda r: r.slice(sp(slab_samples=4097)),
     ValueError, "slab_samples must be 1 .. 4096, not 4097"),
    ("slice/origin-nan", lambda r: r.slice(sp(origin=(nan, 0, 0))),
     ValueError, "slice origin must be finite"),
    ("slice/du-inf", lambda r: r.slice(sp(du=(1, inf, 0))),
     ValueError, "slice du must be finite"),
    ("slice/dv-nan", lambda r: r.slice(sp(dv=(0, 1, nan))),
     ValueError, "slice dv must be finite"),
    ("slice/dn-inf", lambda r: r.slice(sp(dn=(-inf, 0, 1))),
     ValueError, "slice dn must be finite"),
    ("slice/grey-no-window", lambda r: r.slice(sp(), display='grey'),
     ValueError, "display 'grey' needs window = (black, white) with black < white, not None"),
    ("slice/grey-window-reversed", lambda r: r.slice(sp(), display='grey', window=(1.0, 0.0)),
     ValueError, "display 'grey' needs window = (black, white) with black < white, not (1.0, 0.0)"),
    ("slice/grey-window-three", lambda r: r.slice(sp(), display='grey', window=(0.0, 1.0, 2.0)),
     ValueError, "display 'grey' needs window = (black, white) with black < white, not (0.0, 1.0, 2.0)"),
    ("slice/grey-window-nan", lambda r: r.slice(sp(), display='grey', window=(0.0, nan)),
     ValueError, "display 'grey' needs window = (black, white) with black < white, not (0.0, nan)"),
    ("slice/window-without-display", lambda r: r.slice(sp(), window=(0.0, 1.0)),
     ValueError, "window applies to display 'grey' only"),
    ("slice/window-with-tf", lambda r: r.slice(sp(), display='tf', window=(0.0, 1.0)),
     ValueError, "window applies to display 'grey' only"),
    ("slice_mask/not-a-spec", lambda r: r.slice_mask('axial'),
     TypeError, "sp must be a VxSliceParams (volxel_amd.mpr builds them)"),
    ("slice_mask/size-0", lambda r: r.slice_mask(sp(size=(0, 16))),
     ValueError, "slice size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice_mask/size-16385", lambda r: r.slice_mask(sp(size=(16, 16385))),
     ValueError, "slice size must be 1 .. 16384 per side, not 16 x 16385"),
    ("slice_mask/slab-0", lambda r: r.slice_mask(sp(slab_samples=0)),
     ValueError, "slab_samples must be 1 .. 4096, not 0"),
    ("slice_mask/slab-4097", lambda r: r.slice_mask(sp(slab_samples=4097)),
     ValueError, "slab_samples must be 1 .. 4096, not 4097"),
    ("slice_mask/origin-nan", lambda r: r.slice_mask(sp(origin=(nan, 0, 0))),
     ValueError, "slice origin must be finite"),
    ("slice_mask/du-inf", lambda r: r.slice_mask(sp(du=(1, inf, 0))),
     ValueError, "slice du must be finite"),
    ("slice_mask/dv-nan", lambda r: r.slice_mask(sp(dv=(0, 1, nan))),
     ValueError, "slice dv must be finite"),
    ("slice_mask/dn-inf", lambda r: r.slice_mask(sp(dn=(-inf, 0, 1))),
     ValueError, "slice dn must be finite"),
    ("isosurface/iso-nan", lambda r: r.isosurface(nan),
     ValueError, "iso must be finite, not nan"),
    ("isosurface/iso-inf", lambda r: r.isosurface(inf),
     ValueError, "iso must be finite, not inf"),
    ("isosurface/color-two", lambda r: r.isosurface(0.5, color=(1.0, 1.0)),
     ValueError, "color must be three finite values, not (1.0, 1.0)"),
    ("isosurface/color-nan", lambda r: r.isosurface(0.5, color=(1.0, nan, 0.0)),
     ValueError, "color must be three finite values, not (1.0, nan, 0.0)"),
    ("isosurface/phong-three", lambda r: r.isosurface(0.5, phong=(0.3, 0.7, 0.4)),
     ValueError, "phong must be four finite values (ka, kd, ks, shininess), not (0.3, 0.7, 0.4)"),
    ("isosurface/phong-inf", lambda r: r.isosurface(0.5, phong=(0.3, inf, 0.4, 8.0)),
     ValueError, "phong must be four finite values (ka, kd, ks, shininess), not (0.3, inf, 0.4, 8.0)"),
    ("isosurface/shininess-negative", lambda r: r.isosurface(0.5, phong=(0.3, 0.7, 0.4, -1.0)),
     ValueError, "shininess must be >= 0, not -1.0"),
    ("isosurface/refine-17", lambda r: r.isosurface(0.5, refine=17),
     ValueError, "refine must be an integer 0 .. 16, not 17"),
    ("isosurface/refine-negative", lambda r: r.isosurface(0.5, refine=-1),
     ValueError, "refine must be an integer 0 .. 16, not -1"),
    ("isosurface/refine-2.5", lambda r: r.isosurface(0.5, refine=2.5),
     ValueError, "refine must be an integer 0 .. 16, not 2.5"),
    ("isosurface/refine-bool", lambda r: r.isosurface(0.5, refine=True),
     ValueError, "refine must be an integer 0 .. 16, not True"),
    ("isosurface/skip-2", lambda r: r.isosurface(0.5, skip=2),
     ValueError, "skip must be True or False, not 2"),
    ("isosurface/window-empty", lambda r: r.isosurface(0.5, window=(0, 0, 0, 4)),
     ValueError, "window (0, 0, 0, 4) is empty or outside the render size 32 x 24"),
    ("isosurface/window-reversed", lambda r: r.isosurface(0.5, window=(4, 0, 2, 4)),
     ValueError, "window (4, 0, 2, 4) is empty or outside the render size 32 x 24"),
    ("isosurface/window-too-wide", lambda r: r.isosurface(0.5, window=(0, 0, 33, 4)),
     ValueError, "window (0, 0, 33, 4) is empty or outside the render size 32 x 24"),
    ("isosurface/window-too-high", lambda r: r.isosurface(0.5, window=(0, 0, 4, 25)),
     ValueError, "window (0, 0, 4, 25) is empty or outside the render size 32 x 24"),
    ("isosurface/window-three", lambda r: r.isosurface(0.5, window=(0, 0, 4)),
     ValueError, "window must be four integers (x0, y0, x1, y1), not (0, 0, 4)"),
    ("isosurface/window-float", lambda r: r.isosurface(0.5, window=(0, 0.5, 4, 4)),
     ValueError, "window must be four integers (x0, y0, x1, y1), not (0, 0.5, 4, 4)"),
    ("isosurface/pick-outside", lambda r: r.pick(32, 0, 0.5),
     ValueError, "window (32, 0, 33, 1) is empty or outside the render size 32 x 24"),
    ("voxel_index/two", lambda r: r.voxel_index((0.0, 0.0)),
     ValueError, "world_point must be three finite numbers, not (0.0, 0.0)"),
    ("voxel_index/nan", lambda r: r.voxel_index((0.0, nan, 0.0)),
     ValueError, "world_point must be three finite numbers, not (0.0, nan, 0.0)"),
    ("segment_view/unknown", lambda r: setattr(r, 'segment_view', 'glow'),
     VolxelError, "segment_view must be one of ('off', 'only', 'hide'), not 'glow'"),
    ("render_mode/unknown", lambda r: setattr(r, 'render_mode', 'xray'),
     VolxelError, "Unrecognized render mode provided: xray"),
]

PY_NO_VOLUME = [
    ("segment", lambda r: r.segment((1, 1, 1), 0.1),
     VolxelError, "segment: no volume (setup_from_grid first)"),
    ("threshold", lambda r: r.threshold(0.1),
     VolxelError, "threshold: no volume (setup_from_grid first)"),
    ("segment_edit", lambda r: r.segment_edit('dilate'),
     VolxelError, "segment_edit: no volume (setup_from_grid first)"),
    ("set_segment_mask", lambda r: r.set_segment_mask(np.zeros((24, 16, 16), dtype=bool)),
     VolxelError, "set_segment_mask: no volume (setup_from_grid first)"),
    ("islands", lambda r: r.islands(),
     VolxelError, "islands: no volume (setup_from_grid first)"),
    ("keep_largest_islands", lambda r: r.keep_largest_islands(),
     VolxelError, "keep_largest_islands: no volume (setup_from_grid first)"),
    ("remove_small_islands", lambda r: r.remove_small_islands(4),
     VolxelError, "remove_small_islands: no volume (setup_from_grid first)"),
    ("keep_island_at", lambda r: r.keep_island_at((1, 1, 1)),
     VolxelError, "keep_island_at: no volume (setup_from_grid first)"),
    ("island_labels", lambda r: r.island_labels(),
     VolxelError, "island_labels: no volume"),
    ("extract_mesh", lambda r: r.extract_mesh(0.5),
     VolxelError, "extract_mesh: no volume (setup_from_grid first)"),
    ("segment_mask", lambda r: r.segment_mask(),
     VolxelError, "segment_mask: no volume"),
    ("voxel_index", lambda r: r.voxel_index((0.0, 0.0, 0.0)),
     VolxelError, "voxel_index: no volume"),
    ("slice", lambda r: r.slice(sp()),
     VolxelError, "Trying to bind uniforms without a volume."),
    ("isosurface", lambda r: r.isosurface(0.5),
     VolxelError, "Trying to bind uniforms without a volume."),
]

PY_ORDER = [
    ("segment/seed-before-box", "vol", lambda r: r.segment((16, 0, 0), 0.1, box=(1, 2)),
     ValueError, "seed (16, 0, 0) is outside the index extent (16, 16, 24)"),
    ("segment/seed-before-band", "vol", lambda r: r.segment((0, 0), nan),
     ValueError, "seed must be three integer voxel indices (x, y, z), not (0, 0)"),
    ("segment/band-before-connectivity", "vol", lambda r: r.segment((1, 1, 1), 0.5, 0.4, connectivity=18),
     ValueError, "lo = 0.5 > hi = 0.4"),
    ("segment/finite-before-order", "vol", lambda r: r.segment((1, 1, 1), nan, -inf),
     ValueError, "lo and hi must be finite (hi may be inf), not nan, -inf"),
    ("segment/connectivity-before-box", "vol", lambda r: r.segment((1, 1, 1), 0.1, connectivity=18, box=((2, 0, 0), (1, 5, 5))),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("segment/box-before-max-rounds", "vol", lambda r: r.segment((1, 1, 1), 0.1, box=((2, 0, 0), (1, 5, 5)), max_rounds=-1),
     ValueError, "box ((2, 0, 0), (1, 5, 5)) is empty or outside the index extent (16, 16, 24)"),
    ("segment/volume-before-seed", "none", lambda r: r.segment((0, 0), 0.1),
     VolxelError, "segment: no volume (setup_from_grid first)"),
    ("threshold/band-before-box", "vol", lambda r: r.threshold(0.5, 0.4, box=(1, 2)),
     ValueError, "lo = 0.5 > hi = 0.4"),
    ("threshold/volume-before-band", "none", lambda r: r.threshold(nan),
     VolxelError, "threshold: no volume (setup_from_grid first)"),
    ("segment_edit/op-before-connectivity", "vol", lambda r: r.segment_edit('grow', connectivity=18),
     ValueError, "op must be one of ('dilate', 'erode', 'open', 'close', 'fill_holes'), not 'grow'"),
    ("segment_edit/connectivity-before-steps", "vol", lambda r: r.segment_edit('dilate', steps=0, connectivity=18),
     ValueError, "connectivity must be 6 or 26, not 18"),
    ("segment_edit/steps-before-band", "vol", lambda r: r.segment_edit('erode', steps=0, band=True),
     ValueError, "steps must be an integer 1 .. 1024 for erode, not 0"),
    ("segment_edit/volume-before-op", "none", lambda r: r.segment_edit('grow'),
     VolxelError, "segment_edit: no volume (setup_from_grid first)"),
    ("set_segment_mask/dtype-before-shape", "vol", lambda r: r.set_segment_mask(np.zeros(5, dtype=np.uint8)),
     ValueError, "mask must be a bool array, not uint8"),
    ("keep_largest_islands/n-before-connectivity", "vol", lambda r: r.keep_largest_islands(0, connectivity=18),
     ValueError, "n must be an integer >= 1, not 0"),
    ("keep_largest_islands/n-before-volume", "none", lambda r: r.keep_largest_islands(0),
     ValueError, "n must be an integer >= 1, not 0"),
    ("keep_largest_islands/volume-before-connectivity", "none", lambda r: r.keep_largest_islands(1, connectivity=18),
     VolxelError, "keep_largest_islands: no volume (setup_from_grid first)"),
    ("remove_small_islands/min-before-connectivity", "vol", lambda r: r.remove_small_islands(0, connectivity=18),
     ValueError, "min_voxels must be an integer >= 1, not 0"),
    ("keep_island_at/voxel-before-connectivity", "vol", lambda r: r.keep_island_at((16, 0, 0), connectivity=18),
     ValueError, "voxel (16, 0, 0) is outside the index extent (16, 16, 24)"),
    ("keep_island_at/volume-before-voxel", "none", lambda r: r.keep_island_at((0, 0)),
     VolxelError, "keep_island_at: no volume (setup_from_grid first)"),
    ("extract_mesh/space-before-volume", "none", lambda r: r.extract_mesh(0.5, space='mm'),
     ValueError, "space must be one of ('voxel', 'grid', 'world'), not 'mm'"),
    ("extract_mesh/iso-before-box", "vol", lambda r: r.extract_mesh(nan, box=(1, 2)),
     ValueError, "iso must be finite and > 0, not nan"),
    ("extract_mesh/one-of-before-space", "vol", lambda r: r.extract_mesh(space='mm'),
     ValueError, "extract_mesh takes exactly one of iso and segment=True"),
    ("extract_mesh/volume-before-box", "none", lambda r: r.extract_mesh(0.5, box=(1, 2)),
     VolxelError, "extract_mesh: no volume (setup_from_grid first)"),
    ("slice/reduce-before-size", "vol", lambda r: r.slice(sp(size=(0, 16)), reduce='sum'),
     ValueError, "reduce must be one of ['max', 'mean', 'min'], not 'sum'"),
    ("slice/size-before-slab", "vol", lambda r: r.slice(sp(size=(0, 16), slab_samples=0)),
     ValueError, "slice size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice/slab-before-origin", "vol", lambda r: r.slice(sp(slab_samples=0, origin=(nan, 0, 0))),
     ValueError, "slab_samples must be 1 .. 4096, not 0"),
    ("slice/origin-before-dn", "vol", lambda r: r.slice(sp(origin=(nan, 0, 0), dn=(nan, 0, 0))),
     ValueError, "slice origin must be finite"),
    ("slice/spec-before-window", "vol", lambda r: r.slice(sp(dn=(nan, 0, 0)), window=(0.0, 1.0)),
     ValueError, "slice dn must be finite"),
    ("slice/window-before-volume", "none", lambda r: r.slice(sp(), window=(0.0, 1.0)),
     ValueError, "window applies to display 'grey' only"),
    ("slice_mask/size-before-slab", "vol", lambda r: r.slice_mask(sp(size=(0, 16), slab_samples=0)),
     ValueError, "slice size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice_mask/slab-before-origin", "vol", lambda r: r.slice_mask(sp(slab_samples=0, origin=(nan, 0, 0))),
     ValueError, "slab_samples must be 1 .. 4096, not 0"),
    ("isosurface/iso-before-color", "vol", lambda r: r.isosurface(nan, color=(1.0, 1.0)),
     ValueError, "iso must be finite, not nan"),
    ("isosurface/refine-before-window", "vol", lambda r: r.isosurface(0.5, refine=17, window=(0, 0, 0, 4)),
     ValueError, "refine must be an integer 0 .. 16, not 17"),
    ("isosurface/window-before-volume", "none", lambda r: r.isosurface(0.5, window=(0, 0, 0, 4)),
     ValueError, "window (0, 0, 0, 4) is empty or outside the render size 32 x 24"),
    ("voxel_index/volume-before-point", "none", lambda r: r.voxel_index((0.0, 0.0)),
     VolxelError, "voxel_index: no volume"),
]

PY_ACCEPTED = [
    ("segment/max-rounds-1.0", lambda r: r.segment((1, 1, 1), 0.1, max_rounds=1.0)),
    ("segment/seed-whole-floats", lambda r: r.segment((1.0, 2.0, 3.0), 0.1, hi=inf, connectivity=26, box=((0, 0, 0), (15.0, 15, 23)))),
    ("segment/connectivity-6.0", lambda r: r.segment((1, 1, 1), 0.1, connectivity=6.0)),
    ("threshold/lo-equals-hi", lambda r: r.threshold(0.5, 0.5, box=((3, 3, 3), (3, 3, 3)))),
    ("segment_edit/steps-numpy-int", lambda r: r.segment_edit('dilate', steps=np.int64(1024), band=np.bool_(True))),
    ("segment_edit/fill-steps-0", lambda r: r.segment_edit('fill_holes', steps=0)),
    ("set_segment_mask/zyx", lambda r: r.set_segment_mask(np.zeros((24, 16, 16), dtype=bool))),
    ("keep_largest_islands/n-numpy-int", lambda r: r.keep_largest_islands(np.int32(3), connectivity=26)),
    ("remove_small_islands/min-1", lambda r: r.remove_small_islands(1)),
    ("keep_island_at/voxel-whole-floats", lambda r: r.keep_island_at((15.0, 15, 23))),
    ("islands/26", lambda r: r.islands(26)),
    ("extract_mesh/max-vertices-7.0", lambda r: r.extract_mesh(0.5, max_vertices=7.0, space='grid')),
    ("extract_mesh/segment", lambda r: r.extract_mesh(segment=True, box=((0, 0, 0), (0, 0, 0)))),
    ("slice/grey", lambda r: r.slice(sp(slab_samples=4096, size=(16384, 1)), 'max', 'grey', (0.0, 1.0))),
    ("isosurface/refine-8.0", lambda r: r.isosurface(0.5, refine=8.0, skip=1, window=(31, 23, 32, 24))),
]

JS = [
    ("segment/seed-two", "s.segment([0, 0], 0.1)",
     "segment: seed 0,0 is outside the index extent 16,16,24"),
    ("segment/seed-float", "s.segment([0.5, 0, 0], 0.1)",
     "segment: seed 0.5,0,0 is outside the index extent 16,16,24"),
    ("segment/seed-not-an-array", "s.segment('111', 0.1)",
     "segment: seed 111 is outside the index extent 16,16,24"),
    ("segment/seed-x-outside", "s.segment([16, 0, 0], 0.1)",
     "segment: seed 16,0,0 is outside the index extent 16,16,24"),
    ("segment/seed-negative", "s.segment([0, 0, -1], 0.1)",
     "segment: seed 0,0,-1 is outside the index extent 16,16,24"),
    ("segment/lo-nan", "s.segment([1, 1, 1], NaN)",
     "segment: lo and hi must be finite (hi may be Infinity)"),
    ("segment/hi-nan", "s.segment([1, 1, 1], 0.1, { hi: NaN })",
     "segment: lo and hi must be finite (hi may be Infinity)"),
    ("segment/lo-minus-inf", "s.segment([1, 1, 1], -Infinity)",
     "segment: lo and hi must be finite (hi may be Infinity)"),
    ("segment/lo-above-hi", "s.segment([1, 1, 1], 0.5, { hi: 0.4 })",
     "segment: lo = 0.5 > hi = 0.4"),
    ("segment/connectivity-18", "s.segment([1, 1, 1], 0.1, { connectivity: 18 })",
     "segment: connectivity must be 6 or 26, not 18"),
    ("segment/connectivity-string", "s.segment([1, 1, 1], 0.1, { connectivity: '6' })",
     "segment: connectivity must be 6 or 26, not 6"),
    ("segment/box-not-a-pair", "s.segment([1, 1, 1], 0.1, { box: [1, 2] })",
     "segment: box [1,2] is empty or outside the index extent 16,16,24"),
    ("segment/box-one-corner", "s.segment([1, 1, 1], 0.1, { box: [[0, 0, 0]] })",
     "segment: box [[0,0,0]] is empty or outside the index extent 16,16,24"),
    ("segment/box-float", "s.segment([1, 1, 1], 0.1, { box: [[0, 0, 0], [1.5, 2, 2]] })",
     "segment: box [[0,0,0],[1.5,2,2]] is empty or outside the index extent 16,16,24"),
    ("segment/box-empty", "s.segment([1, 1, 1], 0.1, { box: [[2, 0, 0], [1, 5, 5]] })",
     "segment: box [[2,0,0],[1,5,5]] is empty or outside the index extent 16,16,24"),
    ("segment/box-outside", "s.segment([1, 1, 1], 0.1, { box: [[0, 0, 0], [16, 5, 5]] })",
     "segment: box [[0,0,0],[16,5,5]] is empty or outside the index extent 16,16,24"),
    ("segment/max-rounds-negative", "s.segment([1, 1, 1], 0.1, { maxRounds: -1 })",
     "segment: maxRounds must be an integer >= 0"),
    ("segment/max-rounds-2^32", "s.segment([1, 1, 1], 0.1, { maxRounds: 4294967296 })",
     "segment: maxRounds must be an integer >= 0"),
    ("segment/max-rounds-float", "s.segment([1, 1, 1], 0.1, { maxRounds: 1.5 })",
     "segment: maxRounds must be an integer >= 0"),
    ("threshold/lo-nan", "s.threshold(NaN)",
     "threshold: lo and hi must be finite (hi may be Infinity)"),
    ("threshold/hi-minus-inf", "s.threshold(0.1, { hi: -Infinity })",
     "threshold: lo and hi must be finite (hi may be Infinity)"),
    ("threshold/lo-above-hi", "s.threshold(0.5, { hi: 0.4 })",
     "threshold: lo = 0.5 > hi = 0.4"),
    ("threshold/box-not-a-pair", "s.threshold(0.1, { box: [1, 2] })",
     "threshold: box [1,2] is empty or outside the index extent 16,16,24"),
    ("threshold/box-float", "s.threshold(0.1, { box: [[0, 0, 0], [1.5, 2, 2]] })",
     "threshold: box [[0,0,0],[1.5,2,2]] is empty or outside the index extent 16,16,24"),
    ("threshold/box-empty", "s.threshold(0.1, { box: [[2, 0, 0], [1, 5, 5]] })",
     "threshold: box [[2,0,0],[1,5,5]] is empty or outside the index extent 16,16,24"),
    ("threshold/box-outside", "s.threshold(0.1, { box: [[0, 0, 0], [0, 0, 24]] })",
     "threshold: box [[0,0,0],[0,0,24]] is empty or outside the index extent 16,16,24"),
    ("segmentEdit/op-unknown", "s.segmentEdit('grow')",
     "segmentEdit: op must be one of dilate, erode, open, close, fill_holes, not grow"),
    ("segmentEdit/connectivity-18", "s.segmentEdit('dilate', { connectivity: 18 })",
     "segmentEdit: connectivity must be 6 or 26, not 18"),
    ("segmentEdit/connectivity-bool", "s.segmentEdit('dilate', { connectivity: true })",
     "segmentEdit: connectivity must be 6 or 26, not true"),
    ("segmentEdit/steps-0", "s.segmentEdit('dilate', { steps: 0 })",
     "segmentEdit: steps must be an integer 1 .. 1024 for dilate, not 0"),
    ("segmentEdit/steps-1025", "s.segmentEdit('erode', { steps: 1025 })",
     "segmentEdit: steps must be an integer 1 .. 1024 for erode, not 1025"),
    ("segmentEdit/steps-1.5", "s.segmentEdit('open', { steps: 1.5 })",
     "segmentEdit: steps must be an integer 1 .. 1024 for open, not 1.5"),
    ("segmentEdit/fill-steps-2", "s.segmentEdit('fill_holes', { steps: 2 })",
     "segmentEdit: steps must be an integer 0 .. 1 for fill_holes, not 2"),
    ("segmentEdit/band-int", "s.segmentEdit('dilate', { band: 1 })",
     "segmentEdit: band must be a boolean, not 1"),
    ("segmentEdit/band-erode", "s.segmentEdit('erode', { band: true })",
     "segmentEdit: band is for dilate only, not erode"),
    ("setSegmentMask/array", "s.setSegmentMask(new Array(768).fill(0))",
     "setSegmentMask: bits must be a Uint8Array of 768 bytes"),
    ("setSegmentMask/length", "s.setSegmentMask(new Uint8Array(6144))",
     "setSegmentMask: bits must be a Uint8Array of 768 bytes"),
    ("keepLargestIslands/n-0", "s.keepLargestIslands(0)",
     "keepLargestIslands: n must be an integer >= 1, not 0"),
    ("keepLargestIslands/n-1.5", "s.keepLargestIslands(1.5)",
     "keepLargestIslands: n must be an integer >= 1, not 1.5"),
    ("keepLargestIslands/connectivity-18", "s.keepLargestIslands(2, { connectivity: 18 })",
     "keepLargestIslands: connectivity must be 6 or 26, not 18"),
    ("removeSmallIslands/min-0", "s.removeSmallIslands(0)",
     "removeSmallIslands: minVoxels must be an integer >= 1, not 0"),
    ("removeSmallIslands/min-2.5", "s.removeSmallIslands(2.5)",
     "removeSmallIslands: minVoxels must be an integer >= 1, not 2.5"),
    ("removeSmallIslands/connectivity-18", "s.removeSmallIslands(4, { connectivity: 18 })",
     "removeSmallIslands: connectivity must be 6 or 26, not 18"),
    ("keepIslandAt/voxel-two", "s.keepIslandAt([0, 0])",
     "keepIslandAt: voxel 0,0 is outside the index extent 16,16,24"),
    ("keepIslandAt/voxel-float", "s.keepIslandAt([0.5, 0, 0])",
     "keepIslandAt: voxel 0.5,0,0 is outside the index extent 16,16,24"),
    ("keepIslandAt/voxel-x-outside", "s.keepIslandAt([16, 0, 0])",
     "keepIslandAt: voxel 16,0,0 is outside the index extent 16,16,24"),
    ("keepIslandAt/voxel-negative", "s.keepIslandAt([0, 0, -1])",
     "keepIslandAt: voxel 0,0,-1 is outside the index extent 16,16,24"),
    ("keepIslandAt/connectivity-18", "s.keepIslandAt([1, 1, 1], { connectivity: 18 })",
     "keepIslandAt: connectivity must be 6 or 26, not 18"),
    ("islands/connectivity-18", "s.islands({ connectivity: 18 })",
     "islands: connectivity must be 6 or 26, not 18"),
    ("islands/connectivity-bool", "s.islands({ connectivity: true })",
     "islands: connectivity must be 6 or 26, not true"),
    ("extractMesh/segment-int", "s.extractMesh({ segment: 1 })",
     "extractMesh: segment must be a boolean, not 1"),
    ("extractMesh/neither", "s.extractMesh()",
     "extractMesh takes exactly one of iso and segment: true"),
    ("extractMesh/both", "s.extractMesh({ iso: 0.5, segment: true })",
     "extractMesh takes exactly one of iso and segment: true"),
    ("extractMesh/space", "s.extractMesh({ iso: 0.5, space: 'mm' })",
     "extractMesh: space must be one of voxel, grid, world, not mm"),
    ("extractMesh/max-vertices-negative", "s.extractMesh({ iso: 0.5, maxVertices: -1 })",
     "extractMesh: maxVertices must be an integer 0 .. 2^32 - 1, not -1"),
    ("extractMesh/max-triangles-2^32", "s.extractMesh({ iso: 0.5, maxTriangles: 4294967296 })",
     "extractMesh: maxTriangles must be an integer 0 .. 2^32 - 1, not 4294967296"),
    ("extractMesh/iso-nan", "s.extractMesh({ iso: NaN })",
     "extractMesh: iso must be finite and > 0, not NaN"),
    ("extractMesh/iso-zero", "s.extractMesh({ iso: 0 })",
     "extractMesh: iso must be finite and > 0, not 0"),
    ("extractMesh/box-not-a-pair", "s.extractMesh({ iso: 0.5, box: [1, 2] })",
     "extractMesh: box [1,2] is empty or outside the index extent 16,16,24"),
    ("extractMesh/box-float", "s.extractMesh({ iso: 0.5, box: [[0, 0, 0], [1.5, 2, 2]] })",
     "extractMesh: box [[0,0,0],[1.5,2,2]] is empty or outside the index extent 16,16,24"),
    ("extractMesh/box-empty", "s.extractMesh({ segment: true, box: [[2, 0, 0], [1, 5, 5]] })",
     "extractMesh: box [[2,0,0],[1,5,5]] is empty or outside the index extent 16,16,24"),
    ("extractMesh/box-outside", "s.extractMesh({ iso: 0.5, box: [[0, 0, 0], [16, 5, 5]] })",
     "extractMesh: box [[0,0,0],[16,5,5]] is empty or outside the index extent 16,16,24"),
    ("slice/reduce", "s.slice(sp({ reduce: 'sum' }))",
     "slice: reduce must be 'mean', 'max' or 'min', not sum"),
    ("slice/display", "s.slice(sp({ display: 'rgb' }))",
     "slice: display must be null, 'grey' or 'tf', not rgb"),
    ("slice/grey-no-window", "s.slice(sp({ display: 'grey' }))",
     "slice: display grey needs window = [black, white] with black < white"),
    ("slice/grey-window-reversed", "s.slice(sp({ display: 'grey', window: [1, 0] }))",
     "slice: display grey needs window = [black, white] with black < white"),
    ("slice/window-without-display", "s.slice(sp({ window: [0, 1] }))",
     "slice: window applies to display grey only"),
    ("slice/window-with-tf", "s.slice(sp({ display: 'tf', window: [0, 1] }))",
     "slice: window applies to display grey only"),
    ("slice/size-0", "s.slice(sp({ size: [0, 16] }))",
     "slice: size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice/size-16385", "s.slice(sp({ size: [16, 16385] }))",
     "slice: size must be 1 .. 16384 per side, not 16 x 16385"),
    ("slice/origin-two", "s.slice(sp({ origin: [0, 0] }))",
     "uniform origin expects 3 values"),
    ("slice/dn-four", "s.slice(sp({ dn: [0, 0, 1, 0] }))",
     "uniform dn expects 3 values"),
    ("sliceMask/size-0", "s.sliceMask(sp({ size: [0, 16] }))",
     "sliceMask: size must be 1 .. 16384 per side, not 0 x 16"),
    ("sliceMask/size-16385", "s.sliceMask(sp({ size: [16, 16385] }))",
     "sliceMask: size must be 1 .. 16384 per side, not 16 x 16385"),
    ("sliceMask/origin-two", "s.sliceMask(sp({ origin: [0, 0] }))",
     "uniform origin expects 3 values"),
    ("sliceMask/dn-four", "s.sliceMask(sp({ dn: [0, 0, 1, 0] }))",
     "uniform dn expects 3 values"),
    ("isosurface/iso-nan", "s.isosurface(NaN)",
     "isosurface: iso must be finite, not NaN"),
    ("isosurface/iso-inf", "s.isosurface(Infinity)",
     "isosurface: iso must be finite, not Infinity"),
    ("isosurface/color-two", "s.isosurface(0.5, { color: [1, 1] })",
     "isosurface: color must be three finite numbers"),
    ("isosurface/phong-three", "s.isosurface(0.5, { phong: [0.3, 0.7, 0.4] })",
     "isosurface: phong must be [ka, kd, ks, shininess], finite, shininess >= 0"),
    ("isosurface/shininess-negative", "s.isosurface(0.5, { phong: [0.3, 0.7, 0.4, -1] })",
     "isosurface: phong must be [ka, kd, ks, shininess], finite, shininess >= 0"),
    ("isosurface/refine-17", "s.isosurface(0.5, { refine: 17 })",
     "isosurface: refine must be an integer 0 .. 16, not 17"),
    ("isosurface/refine-2.5", "s.isosurface(0.5, { refine: 2.5 })",
     "isosurface: refine must be an integer 0 .. 16, not 2.5"),
    ("isosurface/skip-2", "s.isosurface(0.5, { skip: 2 })",
     "isosurface: skip must be true or false"),
    ("voxelIndex/two", "s.voxelIndex([0, 0])",
     "voxelIndex: w must be three finite numbers"),
    ("voxelIndex/nan", "s.voxelIndex([0, NaN, 0])",
     "voxelIndex: w must be three finite numbers"),
    ("segmentView/unknown", "s.segmentView = 'glow'",
     "segmentView must be one of off, only, hide, not glow"),
    ("renderMode/unknown", "s.renderMode = 'xray'",
     "Unrecognized render mode provided: xray"),
    ("axial/24", "s.axial(24)",
     "k must be a voxel index in [0, 24), not 24"),
    ("axial/negative", "s.axial(-1)",
     "k must be a voxel index in [0, 24), not -1"),
    ("axial/1.5", "s.axial(1.5)",
     "k must be a voxel index in [0, 24), not 1.5"),
    ("coronal/16", "s.coronal(16)",
     "j must be a voxel index in [0, 16), not 16"),
    ("sagittal/16", "s.sagittal(16)",
     "i must be a voxel index in [0, 16), not 16"),
]

JS_NO_VOLUME = [
    ("segment", "n.segment([1, 1, 1], 0.1)",
     "Trying to slice without a volume."),
    ("threshold", "n.threshold(0.1)",
     "Trying to slice without a volume."),
    ("segmentEdit", "n.segmentEdit('dilate')",
     "Trying to bind uniforms without a volume."),
    ("setSegmentMask", "n.setSegmentMask(new Uint8Array(768))",
     "Trying to slice without a volume."),
    ("islands", "n.islands()",
     "Trying to bind uniforms without a volume."),
    ("keepLargestIslands", "n.keepLargestIslands()",
     "Trying to bind uniforms without a volume."),
    ("removeSmallIslands", "n.removeSmallIslands(4)",
     "Trying to bind uniforms without a volume."),
    ("keepIslandAt", "n.keepIslandAt([1, 1, 1])",
     "Trying to slice without a volume."),
    ("islandLabels", "n.islandLabels()",
     "Trying to slice without a volume."),
    ("extractMesh", "n.extractMesh({ iso: 0.5 })",
     "Trying to slice without a volume."),
    ("segmentMask", "n.segmentMask()",
     "Trying to slice without a volume."),
    ("voxelIndex", "n.voxelIndex([0, 0, 0])",
     "voxelIndex: no volume"),
    ("slice", "n.slice(sp({}))",
     "Trying to bind uniforms without a volume."),
    ("isosurface", "n.isosurface(0.5)",
     "Trying to bind uniforms without a volume."),
    ("axial", "n.axial(3)",
     "Trying to slice without a volume."),
    ("coronal", "n.coronal(3)",
     "Trying to slice without a volume."),
    ("sagittal", "n.sagittal(3)",
     "Trying to slice without a volume."),
    ("bindUniforms", "n.bindUniforms()",
     "Trying to bind uniforms without a volume."),
]

JS_ORDER = [
    ("segment/seed-before-box", "s.segment([16, 0, 0], 0.1, { box: [1, 2] })",
     "segment: seed 16,0,0 is outside the index extent 16,16,24"),
    ("segment/seed-before-band", "s.segment([0, 0], NaN)",
     "segment: seed 0,0 is outside the index extent 16,16,24"),
    ("segment/band-before-connectivity", "s.segment([1, 1, 1], 0.5, { hi: 0.4, connectivity: 18 })",
     "segment: lo = 0.5 > hi = 0.4"),
    ("segment/finite-before-order", "s.segment([1, 1, 1], NaN, { hi: -Infinity })",
     "segment: lo and hi must be finite (hi may be Infinity)"),
    ("segment/connectivity-before-box", "s.segment([1, 1, 1], 0.1, { connectivity: 18, box: [[2, 0, 0], [1, 5, 5]] })",
     "segment: connectivity must be 6 or 26, not 18"),
    ("segment/box-before-max-rounds", "s.segment([1, 1, 1], 0.1, { box: [[2, 0, 0], [1, 5, 5]], maxRounds: -1 })",
     "segment: box [[2,0,0],[1,5,5]] is empty or outside the index extent 16,16,24"),
    ("segment/volume-before-seed", "n.segment([0, 0], 0.1)",
     "Trying to slice without a volume."),
    ("threshold/band-before-box", "s.threshold(0.5, { hi: 0.4, box: [1, 2] })",
     "threshold: lo = 0.5 > hi = 0.4"),
    ("threshold/volume-before-band", "n.threshold(NaN)",
     "Trying to slice without a volume."),
    ("segmentEdit/op-before-connectivity", "s.segmentEdit('grow', { connectivity: 18 })",
     "segmentEdit: op must be one of dilate, erode, open, close, fill_holes, not grow"),
    ("segmentEdit/connectivity-before-steps", "s.segmentEdit('dilate', { steps: 0, connectivity: 18 })",
     "segmentEdit: connectivity must be 6 or 26, not 18"),
    ("segmentEdit/steps-before-band", "s.segmentEdit('erode', { steps: 0, band: true })",
     "segmentEdit: steps must be an integer 1 .. 1024 for erode, not 0"),
    ("segmentEdit/op-before-volume", "n.segmentEdit('grow')",
     "segmentEdit: op must be one of dilate, erode, open, close, fill_holes, not grow"),
    ("keepLargestIslands/n-before-connectivity", "s.keepLargestIslands(0, { connectivity: 18 })",
     "keepLargestIslands: n must be an integer >= 1, not 0"),
    ("keepLargestIslands/connectivity-before-volume", "n.keepLargestIslands(1, { connectivity: 18 })",
     "keepLargestIslands: connectivity must be 6 or 26, not 18"),
    ("removeSmallIslands/min-before-connectivity", "s.removeSmallIslands(0, { connectivity: 18 })",
     "removeSmallIslands: minVoxels must be an integer >= 1, not 0"),
    ("keepIslandAt/voxel-before-connectivity", "s.keepIslandAt([16, 0, 0], { connectivity: 18 })",
     "keepIslandAt: voxel 16,0,0 is outside the index extent 16,16,24"),
    ("keepIslandAt/volume-before-voxel", "n.keepIslandAt([0, 0])",
     "Trying to slice without a volume."),
    ("extractMesh/space-before-volume", "n.extractMesh({ iso: 0.5, space: 'mm' })",
     "extractMesh: space must be one of voxel, grid, world, not mm"),
    ("extractMesh/iso-before-box", "s.extractMesh({ iso: NaN, box: [1, 2] })",
     "extractMesh: iso must be finite and > 0, not NaN"),
    ("extractMesh/one-of-before-space", "s.extractMesh({ space: 'mm' })",
     "extractMesh takes exactly one of iso and segment: true"),
    ("extractMesh/volume-before-box", "n.extractMesh({ iso: 0.5, box: [1, 2] })",
     "Trying to slice without a volume."),
    ("slice/reduce-before-size", "s.slice(sp({ reduce: 'sum', size: [0, 16] }))",
     "slice: reduce must be 'mean', 'max' or 'min', not sum"),
    ("slice/window-before-size", "s.slice(sp({ window: [0, 1], size: [0, 16] }))",
     "slice: window applies to display grey only"),
    ("slice/size-before-origin", "s.slice(sp({ size: [0, 16], origin: [0, 0] }))",
     "slice: size must be 1 .. 16384 per side, not 0 x 16"),
    ("slice/origin-before-dn", "s.slice(sp({ origin: [0, 0], dn: [0, 0] }))",
     "uniform origin expects 3 values"),
    ("slice/origin-before-volume", "n.slice(sp({ origin: [0, 0] }))",
     "uniform origin expects 3 values"),
    ("sliceMask/size-before-origin", "s.sliceMask(sp({ size: [0, 16], origin: [0, 0] }))",
     "sliceMask: size must be 1 .. 16384 per side, not 0 x 16"),
    ("sliceMask/du-before-dv", "s.sliceMask(sp({ du: [0, 0], dv: [0, 0] }))",
     "uniform du expects 3 values"),
    ("isosurface/iso-before-color", "s.isosurface(NaN, { color: [1, 1] })",
     "isosurface: iso must be finite, not NaN"),
    ("isosurface/refine-before-skip", "s.isosurface(0.5, { refine: 17, skip: 2 })",
     "isosurface: refine must be an integer 0 .. 16, not 17"),
    ("isosurface/skip-before-volume", "n.isosurface(0.5, { skip: 2 })",
     "isosurface: skip must be true or false"),
    ("voxelIndex/volume-before-point", "n.voxelIndex([0, 0])",
     "voxelIndex: no volume"),
]

JS_ACCEPTED = [
    ("segment", "b.segment([15, 15, 23], 0.1, { hi: Infinity, connectivity: 26, box: [[0, 0, 0], [15, 15, 23]], maxRounds: 4294967295 })"),
    ("threshold", "b.threshold(0.5, { hi: 0.5, box: [[3, 3, 3], [3, 3, 3]] })"),
    ("segmentEdit", "b.segmentEdit('dilate', { steps: 1024, band: true })"),
    ("segmentEdit/fill-steps-0", "b.segmentEdit('fill_holes', { steps: 0 })"),
    ("setSegmentMask", "b.setSegmentMask(new Uint8Array(768))"),
    ("keepLargestIslands", "b.keepLargestIslands(3, { connectivity: 26 })"),
    ("removeSmallIslands", "b.removeSmallIslands(1)"),
    ("keepIslandAt", "b.keepIslandAt([15, 15, 23])"),
    ("islands", "b.islands({ connectivity: 26 })"),
    ("extractMesh", "b.extractMesh({ segment: true, box: [[0, 0, 0], [0, 0, 0]], space: 'grid', maxVertices: 4294967295 })"),
    ("slice", "b.slice(sp({ size: [16384, 1], slabSamples: 4096, reduce: 'max', display: 'grey', window: [0, 1] }))"),
    ("isosurface", "b.isosurface(0.5, { refine: 16, skip: false })"),
]


# ---- Python ------------------------------------------------------------------------------------------------------------
def _py_mismatches(cases):
    bad = []
    for case in cases:
        (name, kind, call, typ, msg) = case if len(case) == 5 else (case[0], None, *case[1:])
        try:
            call(shell(kind))
            bad.append((name, "no refusal"))
        except Exception as e:
            if type(e) is not typ or str(e) != msg:
                bad.append((name, type(e).__name__, str(e)))
    return bad


def test_python_refusals():
    assert _py_mismatches([(n, "vol", c, t, m) for n, c, t, m in PY]) == []


def test_python_refusals_without_a_volume():
    assert _py_mismatches([(n, "none", c, t, m) for n, c, t, m in PY_NO_VOLUME]) == []


def test_python_first_check_wins():
    assert _py_mismatches(PY_ORDER) == []


def test_python_calls_that_pass_every_check():
    assert _py_mismatches([(n, "bound", c, Bound, "bind_uniforms") for n, c in PY_ACCEPTED]) == []


def test_python_shared_checks_are_covered_per_method():
    """every method that makes a shared check has a case of it, with the same text after the argument's name"""
    texts = {n: m for n, _, _, m in PY}
    for method in ("segment", "threshold", "extract_mesh"):
        for case in ("box-not-a-pair", "box-float", "box-empty"):
            assert texts[f"{method}/{case}"] == texts[f"segment/{case}"], (method, case)
    for method in ("segment", "threshold"):
        for case in ("lo-nan", "lo-above-hi"):
            assert texts[f"{method}/{case}"] == texts[f"segment/{case}"], (method, case)
    for method in ("segment", "segment_edit", "keep_largest_islands", "remove_small_islands", "keep_island_at", "islands"):
        assert texts[f"{method}/connectivity-18"] == "connectivity must be 6 or 26, not 18", method
    for a, b in (("seed-two", "voxel-two"), ("seed-float", "voxel-float"), ("seed-x-outside", "voxel-x-outside")):
        assert texts[f"segment/{a}"].replace("seed", "voxel") == texts[f"keep_island_at/{b}"]
    for case in ("not-a-spec", "size-0", "slab-0", "origin-nan", "dn-inf"):
        assert texts[f"slice/{case}"] == texts[f"slice_mask/{case}"], case


# ---- JavaScript --------------------------------------------------------------------------------------------------------
# in scope for a case: s (a shell with the (16, 16, 24) volume description), n (one without a volume), b (one whose bindUniforms
# throws 'bindUniforms') and sp(fields), the axial plane k = 3 as a slice spec with some fields replaced
JS_PRELUDE = r"""
const v = require(process.argv[2]);
const shell = (volume) => Object.assign(Object.create(v.Volxel3DDicomRenderer.prototype),
  { volume, settings: { phong: [0.3, 0.7, 0.4, 32] }, width: 32, height: 24 });
const sp = (o) => Object.assign({ origin: [0, 0, 3], du: [1, 0, 0], dv: [0, 1, 0], dn: [0, 0, 1], size: [16, 16], slabSamples: 1 }, o);
const out = {};
const refusal = (id, f) => {
  const s = shell({ grid: { indexExtent: [16, 16, 24] } }), n = shell(null), b = shell({ grid: { indexExtent: [16, 16, 24] } });
  b.bindUniforms = () => { throw new Error('bindUniforms'); };
  try { f(s, n, b); out[id] = null; } catch (e) { out[id] = e.message; }
};
"""

needs_node = pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")


def _js_messages(tmp_path, cases):
    """{id: the message the call threw, or None} from one node process"""
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = tmp_path / "refusals.js"
    script.write_text(JS_PRELUDE + "".join(f"refusal({json.dumps(c[0])}, (s, n, b) => {{ {c[1]}; }});\n" for c in cases)
                      + "console.log(JSON.stringify(out));\n")
    out = subprocess.run(["node", str(script), NAPI], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@needs_node
def test_js_refusals(native_lib, tmp_path):
    assert _js_messages(tmp_path, JS) == {n: m for n, _, m in JS}


@needs_node
def test_js_refusals_without_a_volume(native_lib, tmp_path):
    assert _js_messages(tmp_path, JS_NO_VOLUME) == {n: m for n, _, m in JS_NO_VOLUME}


@needs_node
def test_js_first_check_wins(native_lib, tmp_path):
    assert _js_messages(tmp_path, JS_ORDER) == {n: m for n, _, m in JS_ORDER}


@needs_node
def test_js_calls_that_pass_every_check(native_lib, tmp_path):
    assert _js_messages(tmp_path, JS_ACCEPTED) == {n: "bindUniforms" for n, _ in JS_ACCEPTED}


def test_js_shared_checks_are_covered_per_method():
    """every method that makes a shared check has a case of it, with the same text after the method's name"""
    texts = {n: m for n, _, m in JS}
    rest = lambda k: texts[k].split(": ", 1)[1]
    for method in ("segment", "threshold", "extractMesh"):
        for case in ("box-not-a-pair", "box-float", "box-empty"):
            assert texts[f"{method}/{case}"].startswith(method + ": ") and rest(f"{method}/{case}") == rest(f"segment/{case}")
    for case in ("lo-nan", "lo-above-hi"):
        assert texts[f"threshold/{case}"].startswith("threshold: ") and rest(f"threshold/{case}") == rest(f"segment/{case}")
    for method in ("segment", "segmentEdit", "keepLargestIslands", "removeSmallIslands", "keepIslandAt", "islands"):
        assert texts[f"{method}/connectivity-18"] == f"{method}: connectivity must be 6 or 26, not 18"
    for a, b in (("seed-two", "voxel-two"), ("seed-float", "voxel-float"), ("seed-x-outside", "voxel-x-outside")):
        assert rest(f"segment/{a}").replace("seed", "voxel") == rest(f"keepIslandAt/{b}")
    for case in ("size-0", "size-16385", "origin-two", "dn-four"):
        assert texts[f"slice/{case}"].replace("slice: ", "") == texts[f"sliceMask/{case}"].replace("sliceMask: ", "")
