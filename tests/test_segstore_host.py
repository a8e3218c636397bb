"""The segment store without a device (DESIGN.md section 2 "Segment store"): the restatement (tests/segstore_ref.py) against set
algebra, against the brute-force distance definition and against SciPy's float64 transform; and the hosts' plumbing: struct
layouts, enums, exports, the new addon's boundary, refusals.  CPU only."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests import distance_ref as DR
from tests import segedit_ref as ER
from tests import segstore_ref as SS
from tests.common import NAPI, ROOT
from tests.shapes import offsets, renderer_shell

# the small masks and spacings the distance restatement is pinned on (tests/test_distance_host.py)
SHAPE = (11, 13, 17)     # z, y, x
SPACINGS = {"unit": (1.0, 1.0, 1.0), "ct": (0.5, 0.5, 2.0), "ragged": (0.7, 0.9, 2.5), "mixed": (0.3, 1.1, 0.9)}


def _masks():
    rng = np.random.default_rng(20250301)
    sparse = rng.random(SHAPE) < 0.02
    dense = rng.random(SHAPE) < 0.4
    one = np.zeros(SHAPE, dtype=bool)
    one[0, 0, 0] = True
    return {"sparse": sparse, "dense": dense, "corner": one, "blobs": ER.blobs(SHAPE, seed=3, sigma=1.5, q=0.7)}


MASKS = _masks()
PAIRS = [("sparse", "dense"), ("blobs", "sparse"), ("corner", "blobs"), ("dense", "dense")]
EMPTY, FULL = np.zeros(SHAPE, dtype=bool), np.ones(SHAPE, dtype=bool)


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
def test_set_algebra_identities_on_random_masks():
    rng = np.random.default_rng(7)
    for _ in range(4):
        A, B, Cm = (rng.random((9, 10, 12)) < p for p in (0.3, 0.5, 0.7))
        u, i, s, x, n = (SS.combine(op, A, B) for op in SS.OPS)
        assert np.array_equal(u, SS.combine("union", B, A)) and np.array_equal(i, SS.combine("intersect", B, A))
        assert np.array_equal(x, SS.combine("union", s, SS.combine("subtract", B, A))) and not (s & B).any()
        assert np.array_equal(u, SS.combine("xor", x, i)) and np.array_equal(s, SS.combine("intersect", A, SS.combine("invert", B)))
        assert np.array_equal(SS.combine("invert", n), A) and n.sum() == A.size - A.sum()
        # De Morgan, distributivity, inclusion-exclusion
        assert np.array_equal(SS.combine("invert", u), SS.combine("intersect", n, SS.combine("invert", B)))
        assert np.array_equal(SS.combine("intersect", A, SS.combine("union", B, Cm)),
                              SS.combine("union", i, SS.combine("intersect", A, Cm)))
        a, b, both = SS.counts(A, B)
        assert int(u.sum()) == a + b - both and int(x.sum()) == a + b - 2 * both and int(s.sum()) == a - both
        assert SS.dice(a, b, both) == 2 * both / (a + b) and SS.jaccard(a, b, both) == both / int(u.sum())
        for op in ("union", "intersect"):
            assert np.array_equal(SS.combine(op, A, A), A)
        assert not SS.combine("xor", A, A).any() and not SS.combine("subtract", A, A).any()
    assert math.isnan(SS.dice(0, 0, 0)) and math.isnan(SS.jaccard(0, 0, 0))
    assert SS.dice(5, 5, 5) == 1.0 == SS.jaccard(5, 5, 5) and SS.dice(3, 4, 0) == 0.0 == SS.jaccard(3, 4, 0)
    with pytest.raises(ValueError):
        SS.combine("nand", EMPTY, EMPTY)


@pytest.mark.parametrize("sp", sorted(SPACINGS))
@pytest.mark.parametrize("a, b", PAIRS)
def test_hausdorff_against_the_brute_force_definition(a, b, sp):
    """bit for bit: the field route of the restatement against one candidate at a time, both directions, voxel included"""
    A, B, s = MASKS[a], MASKS[b], SPACINGS[sp]
    for own, other in ((A, B), (B, A)):
        v, at = SS.directed(own, other, s)
        bv, bat = SS.directed(own, other, s, f=DR.brute)
        assert v.view(np.uint32) == bv.view(np.uint32) and at == bat
        # the definition spelled out: the largest over `own` of the smallest over `other`
        d2 = DR.brute(other, s)
        assert v == d2[own].max() and own[at[2], at[1], at[0]] and d2[at[2], at[1], at[0]] == v
        first = np.flatnonzero((own & (d2 == v)).ravel())[0]
        assert at == tuple(int(q) for q in np.unravel_index(first, SHAPE)[::-1])
    if a == b:
        assert SS.directed(A, B, s)[0] == 0.0


@pytest.mark.parametrize("sp", sorted(SPACINGS))
@pytest.mark.parametrize("a, b", PAIRS)
def test_hausdorff_against_scipy(a, b, sp):
    """|D2 - e^2| <= 5 * 2^-24 * e^2, the bound tests/test_distance_host.py holds the field to (three roundings in a term and
    two in the sums); the max over a set of values each within the bound is within it"""
    A, B, s = MASKS[a], MASKS[b], SPACINGS[sp]
    for own, other in ((A, B), (B, A)):
        e = ndimage.distance_transform_edt(~other, sampling=s[::-1])
        want = float((e[own] ** 2).max())
        got = float(SS.directed(own, other, s)[0])
        print(f"{a} {b} {sp}: {got} against {want}, relative {abs(got - want) / want if want else 0.0:.3e}")
        assert abs(got - want) <= 5 * 2.0 ** -24 * want


def test_the_empty_set_conventions():
    s = SPACINGS["ct"]
    A = MASKS["blobs"]
    first = tuple(int(q) for q in np.unravel_index(np.flatnonzero(A.ravel())[0], SHAPE)[::-1])
    assert SS.directed(EMPTY, A, s) == (0.0, (0, 0, 0)) and SS.directed(EMPTY, EMPTY, s) == (0.0, (0, 0, 0))
    v, at = SS.directed(A, EMPTY, s)
    assert np.isinf(v) and v > 0 and at == first
    assert SS.directed(A, FULL, s) == (0.0, first)            # every voxel of A is in the other set: the first of equal maxima
    assert SS.directed(FULL, A, s)[0] == DR.field(A, s).max() > 0


def test_label_map_priority_is_list_order():
    rng = np.random.default_rng(3)
    m = [rng.random((6, 7, 9)) < 0.4 for _ in range(3)]
    lab, over = SS.labelmap(m)
    assert lab.dtype == np.uint8 and over == int(((m[0].astype(int) + m[1] + m[2]) > 1).sum()) > 0
    assert np.array_equal(lab == 1, m[0]) and np.array_equal(lab == 2, m[1] & ~m[0]) and np.array_equal(lab == 3, m[2] & ~m[1] & ~m[0])
    assert np.array_equal(lab == 0, ~(m[0] | m[1] | m[2]))
    rev, over_rev = SS.labelmap(m[::-1])
    assert over_rev == over and np.array_equal(rev == 1, m[2]) and not np.array_equal(rev == 3, lab == 1)
    assert SS.labelmap([m[0]])[1] == 0 and SS.labelmap([m[0], ~m[0]])[1] == 0 and (SS.labelmap([m[0], ~m[0]])[0] > 0).all()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxCombineParams, VxCompareParams, VxCompareResult
    for cls, names, want in (
            (VxCombineParams, ["op", "slot"], [8, 0, 4]),
            (VxCompareParams, ["slot", "hausdorff", "spacing"], [20, 0, 4, 8]),
            (VxCompareResult, ["count_a", "count_b", "count_and", "d2_ab", "d2_ba", "argmax_ab", "argmax_ba"],
             [56, 0, 8, 16, 24, 28, 32, 44])):
        assert cls is getattr(_abi, cls.__name__)
        assert [f[0] for f in cls._fields_] == names
        got = offsets(tmp_path, cls.__name__, names)
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n in names] == want


def test_enums_match_the_header():
    from volxel_amd import _abi
    from volxel_amd.renderer import Volxel3DRenderer
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    for name, value in _abi.COMBINE_OPS.items():
        assert int(re.search(r"VX_COMBINE_%s = (\d+)" % name.upper(), text).group(1)) == value
    assert Volxel3DRenderer.COMBINE_OPS == tuple(sorted(_abi.COMBINE_OPS, key=_abi.COMBINE_OPS.get)) == SS.OPS
    assert int(re.search(r"#define VX_SEGMENT_SLOTS (\d+)u", text).group(1)) == _abi.SEGMENT_SLOTS == 32


ENTRY_POINTS = ("vx_segment_store", "vx_segment_load", "vx_segment_drop", "vx_segment_slots", "vx_segment_combine",
                "vx_segment_compare", "vx_segments_labelmap")
JS_METHODS = {"storeSegment": 2, "loadSegment": 2, "dropSegment": 2, "storedSegments": 1, "segmentCombine": 3, "segmentCompare": 6,
              "segmentsLabelmap": 3}          # the addon's functions and how many arguments each takes


def test_entry_points_are_declared_exported_and_bound_in_both_hosts(native_lib):
    from volxel_amd import _abi
    napi = os.path.join(ROOT, "volxel_amd", "napi")
    c = open(os.path.join(napi, "volxel_napi_segments.c")).read()      # the addon of the segment store
    js = open(os.path.join(napi, "viewer.js")).read()
    dts = open(os.path.join(napi, "index.d.ts")).read()
    for name in ENTRY_POINTS:
        assert name in _abi.declared_symbols("volxel_hip.h")
        assert getattr(native_lib, name).argtypes is not None              # bound with a signature by load_library
        assert name + "(" in c
    for m in JS_METHODS:
        assert f"  {m}(" in js and f"  {m}(" in dts and f'"{m}"' in c
    for word in SS.OPS:
        assert f"'{word}'" in js and f"'{word}'" in dts
    assert "volxel_napi_segments.node" in open(os.path.join(napi, "Makefile")).read()


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_segments_addon_boundary(tmp_path):
    """volxel_napi_segments.node: its exported names and its argument-count and handle guards; no device is touched: every call
    here is refused before the C ABI is reached.  The two other addons keep the exports they had."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "volxel_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = r"""
const path = require('path');
const native = require(path.join(process.argv[2], 'volxel_napi_segments.node'));
const arity = JSON.parse(process.argv[3]);
const thrown = (f) => { try { f(); return null; } catch (e) { return { type: e instanceof TypeError, msg: e.message }; } };
const out = { keys: Object.keys(native).sort(), none: {}, short: {}, handle: {},
              others: [...Object.keys(require(path.join(process.argv[2], 'volxel_napi.node'))),
                       ...Object.keys(require(path.join(process.argv[2], 'volxel_napi_distance.node')))] };
for (const k of out.keys) {
  out.none[k] = thrown(() => native[k]());
  out.short[k] = thrown(() => native[k](...new Array(arity[k] - 1).fill({})));   // one argument too few
  out.handle[k] = thrown(() => native[k]({}, ...new Array(arity[k] - 1).fill(0)));
}
console.log(JSON.stringify(out));
"""
    (tmp_path / "b.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "b.js"), NAPI, json.dumps(JS_METHODS)], timeout=120))
    assert out["keys"] == sorted(JS_METHODS) and not set(JS_METHODS) & set(out["others"])
    for k in JS_METHODS:
        for kind in ("none", "short"):
            e = out[kind][k]
            assert e is not None and e["type"] and "wrong number of arguments" in e["msg"], (k, kind, e)
        e = out["handle"][k]
        assert e is not None and e["type"] and "expected a context handle" in e["msg"], (k, e)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    invalid = int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))
    cb, cp = _abi.VxCombineParams(), _abi.VxCompareParams()
    buf = np.zeros(8, dtype=np.uint8)
    slots = (C.c_uint32 * 1)(0)
    occ = C.c_uint32()
    assert native_lib.vx_segment_store(None, 0) == invalid
    assert native_lib.vx_segment_load(None, 0, None) == invalid
    assert native_lib.vx_segment_drop(None, 0) == invalid
    assert native_lib.vx_segment_slots(None, C.byref(occ)) == invalid
    assert native_lib.vx_segment_combine(None, C.byref(cb), None) == invalid
    assert native_lib.vx_segment_compare(None, C.byref(cp), None) == invalid
    assert native_lib.vx_segments_labelmap(None, slots, 1, buf.ctypes.data, 8, None) == invalid


BAD_SLOTS = [-1, 32, 1.5, True, "0"]


@pytest.mark.parametrize("bad", BAD_SLOTS, ids=[repr(b) for b in BAD_SLOTS])
def test_python_refusals_of_a_bad_slot(bad):
    r = renderer_shell()
    calls = (lambda: r.store_segment(bad), lambda: r.load_segment(bad), lambda: r.drop_segment(bad),
             lambda: r.segment_combine("union", bad), lambda: r.segment_compare(bad), lambda: r.segment_compare(bad, hausdorff=False),
             lambda: r.segments_labelmap([0, bad]))
    for call in calls:
        with pytest.raises(ValueError, match="slot"):
            call()


@pytest.mark.parametrize("call, word", [
    (lambda r: r.segment_combine("nand", 0), "op"), (lambda r: r.segment_combine(0, 0), "op"),
    (lambda r: r.segment_combine("invert", 0), "slot"), (lambda r: r.segment_combine("union"), "slot"),
    (lambda r: r.segment_combine("subtract", None), "slot"),
    (lambda r: r.segments_labelmap([]), "slots"), (lambda r: r.segments_labelmap(list(range(32)) + [0]), "slots"),
    (lambda r: r.segments_labelmap([3, 5, 3]), "slots"), (lambda r: r.segments_labelmap(4), "slots"),
    (lambda r: r.segment_compare(0, hausdorff=1), "hausdorff"),
    (lambda r: r.segment_compare(0, spacing=(1.0, 1.0)), "spacing"), (lambda r: r.segment_compare(0, spacing=(1.0, 0.0, 1.0)), "spacing"),
    (lambda r: r.segment_compare(0, spacing=(1.0, float("nan"), 1.0)), "spacing"),
    (lambda r: r.segment_compare(0, hausdorff=False, spacing=(1.0, -1.0, 1.0)), "spacing"),
], ids=["op-unknown", "op-number", "invert-slot", "union-none", "subtract-none", "list-empty", "list-long", "list-duplicate",
        "list-scalar", "hausdorff", "spacing-short", "spacing-zero", "spacing-nan", "spacing-negative"])
def test_python_refusals_by_argument_name(call, word):
    with pytest.raises(ValueError, match=word):
        call(renderer_shell())


def test_no_volume_is_refused_by_name():
    from volxel_amd import VolxelError
    r = renderer_shell()
    r.volume = None
    for call, name in ((lambda: r.store_segment(0), "store_segment"), (lambda: r.load_segment(0), "load_segment"),
                       (lambda: r.drop_segment(0), "drop_segment"), (lambda: r.stored_segments(), "stored_segments"),
                       (lambda: r.segment_combine("invert"), "segment_combine"), (lambda: r.segment_compare(0), "segment_compare"),
                       (lambda: r.segments_labelmap([0]), "segments_labelmap")):
        with pytest.raises(VolxelError, match=name):
            call()


def test_the_shared_slot_checks():
    from volxel_amd import _checks
    assert _checks.slot(0) == 0 and _checks.slot(31) == 31 and _checks.slot(np.int64(7)) == 7
    assert _checks.slots([3, 0, 31]) == (3, 0, 31) and _checks.slots(np.arange(32)) == tuple(range(32))
    assert _checks.slots((5,)) == (5,)
