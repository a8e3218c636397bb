"""The distance field and the margins without a device (DESIGN.md section 2 "Distances and margins"): the restatement
(tests/distance_ref.py) against itself -- brute force == separable == windowed, bit for bit -- and against SciPy's float64
Euclidean transform; the margins against SciPy's balls where no tie can occur and against the voxel-count edits where the two
agree; and the hosts' plumbing: struct layouts, enums, exports, refusals, the default spacing.  CPU only."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
from scipy import ndimage

from tests import distance_ref as DR
from tests import segedit_ref as ER
from tests.common import F32, NAPI, ROOT
from tests.shapes import offsets, renderer_shell

SHAPE = (11, 13, 17)     # z, y, x
SPACINGS = {"unit": (1.0, 1.0, 1.0), "ct": (0.5, 0.5, 2.0), "ragged": (0.7, 0.9, 2.5), "mixed": (0.3, 1.1, 0.9)}
# a fraction of a voxel (of the finest axis), a few voxels, no cap
CAPS = {"fraction": lambda sp: 0.6 * min(sp), "few": lambda sp: 3.3 * max(sp), "inf": lambda sp: np.inf}


def _masks():
    rng = np.random.default_rng(20250301)
    sparse = rng.random(SHAPE) < 0.02
    dense = rng.random(SHAPE) < 0.4
    one = np.zeros(SHAPE, dtype=bool)
    one[0, 0, 0] = True
    return {"sparse": sparse, "dense": dense, "corner": one, "blobs": ER.blobs(SHAPE, seed=3, sigma=1.5, q=0.7)}


MASKS = _masks()
_BRUTE = {}


def _brute(mask, sp):
    if (mask, sp) not in _BRUTE:
        _BRUTE[mask, sp] = DR.brute(MASKS[mask], SPACINGS[sp])
    return _BRUTE[mask, sp]


def bits(a):
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


# ---- the restatement against itself ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", sorted(SPACINGS))
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_brute_force_separable_and_windowed_agree_bit_for_bit(mask, sp):
    S, s = MASKS[mask], SPACINGS[sp]
    b = _brute(mask, sp)
    assert np.isfinite(b).all() and (b[S] == 0).all() and (b[~S] > 0).all()
    assert np.array_equal(bits(DR.separable(S, s)), bits(b))
    assert np.array_equal(bits(DR.field(S, s)), bits(b))                   # the index-scan x pass the GPU tests' reference uses
    for cap in sorted(CAPS):
        r = CAPS[cap](s)
        want = DR.capped(b, DR.cap2(r))
        w = DR.windowed(S, s, r)
        assert np.array_equal(bits(w), bits(want)), (cap, int((bits(w) != bits(want)).sum()))
        assert np.array_equal(bits(DR.field(S, s, r)), bits(want))
        if cap == "fraction":
            assert np.array_equal(np.isfinite(want), S)                    # under one voxel: only the sources are in reach
        if cap == "few":
            assert (np.isfinite(want) & ~S).any()


def test_the_empty_source_set_is_infinitely_far():
    S = np.zeros(SHAPE, dtype=bool)
    for f in (DR.brute, DR.separable, DR.field):
        assert np.isinf(f(S, SPACINGS["ct"])).all()
    assert np.isinf(DR.windowed(S, SPACINGS["ct"], 3.0)).all()
    assert DR.stats(DR.field(S, SPACINGS["ct"]), S) == (0, 0.0, (0, 0, 0))
    full = ~S
    assert DR.stats(DR.field(full, SPACINGS["ct"]), full) == (full.size, 0.0, (0, 0, 0))


def test_windows_follow_the_cap():
    for s in (1.0, 0.5, 0.7, 2.5):
        for r in (0.2, 1.0, 2.3, 7.9):
            r2 = DR.cap2(r)
            w = DR.window(s, r2, 64)
            assert DR.term(w, s) <= r2 < DR.term(w + 1, s)
    assert DR.window(1.0, DR.cap2(np.inf), 17) == 16


# ---- against SciPy --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sp", sorted(SPACINGS))
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_field_against_scipy(mask, sp):
    """|D2 - e^2| <= 5 * 2^-24 * e^2 = 3.0e-7 e^2: three roundings in a term and two in the sums.  Measured: 1.8e-7 on the two
    ragged spacings, exact on the other two (each case prints its figure)."""
    S, s = MASKS[mask], SPACINGS[sp]
    e = ndimage.distance_transform_edt(~S, sampling=s[::-1])               # float64, (z, y, x) sampling
    d2 = _brute(mask, sp).astype(np.float64)
    err = np.abs(d2 - e * e)
    rel = float((err[e > 0] / (e * e)[e > 0]).max())
    print(f"{mask} {sp}: max relative error {rel:.3e}")
    assert (err <= 5 * 2.0 ** -24 * e * e).all(), rel


# (spacing, radius): every D2 is an integer or a multiple of 0.25 and the radius squared (6.25, 5.29) is not: no tie
NO_TIE = {"unit": 2.5, "ct": 2.3}


@pytest.mark.parametrize("sp", sorted(NO_TIE))
@pytest.mark.parametrize("mask", sorted(MASKS))
def test_margin_sets_against_scipy(mask, sp):
    M, s, r = MASKS[mask], SPACINGS[sp], NO_TIE[sp]
    out = ndimage.distance_transform_edt(~M, sampling=s[::-1])
    # scipy measures to the nearest False voxel inside the array: the border rule of SHRINK (outside counts as set)
    grow = out <= r
    assert np.array_equal(DR.margin(M, "grow", r, s), grow)
    shrink = M & ~(ndimage.distance_transform_edt(M, sampling=s[::-1]) <= r) if not M.all() else M
    assert np.array_equal(DR.margin(M, "shrink", r, s), shrink)
    close = grow & ~(ndimage.distance_transform_edt(grow, sampling=s[::-1]) <= r) if not grow.all() else grow
    assert np.array_equal(DR.margin(M, "close", r, s), close)
    opened = ndimage.distance_transform_edt(~shrink, sampling=s[::-1]) <= r if shrink.any() else shrink
    assert np.array_equal(DR.margin(M, "open", r, s), opened)
    for f in (DR.brute, DR.separable):                                     # the ops on the definition itself
        assert np.array_equal(DR.margin(M, "grow", r, s, f=f), grow)
        assert np.array_equal(DR.margin(M, "shrink", r, s, f=f), shrink)


# ---- algebra --------------------------------------------------------------------------------------------------------------------
ALGEBRA_MASKS = {"blobs": ER.blobs((20, 22, 26), seed=9, sigma=2.0, q=0.75), "dense": np.random.default_rng(4).random((12, 14, 18)) < 0.5}


@pytest.mark.parametrize("mask", sorted(ALGEBRA_MASKS))
def test_unit_margins_are_the_voxel_edits(mask):
    m = ALGEBRA_MASKS[mask]
    one = (1.0, 1.0, 1.0)
    assert np.array_equal(DR.margin(m, "grow", 1.0, one), ER.edit(m, "dilate", 6, 1))
    assert np.array_equal(DR.margin(m, "grow", 1.75, one), ER.edit(m, "dilate", 26, 1))
    assert np.array_equal(DR.margin(m, "shrink", 1.0, one), ER.edit(m, "erode", 6, 1))
    assert np.array_equal(DR.margin(m, "shrink", 1.75, one), ER.edit(m, "erode", 26, 1))
    assert (DR.margin(m, "grow", 1.0, one) ^ m).any() and (DR.margin(m, "shrink", 1.0, one) ^ m).any()


@pytest.mark.parametrize("sp", ["unit", "ct", "ragged"])
@pytest.mark.parametrize("mask", sorted(ALGEBRA_MASKS))
def test_close_is_extensive_open_anti_extensive_both_idempotent(mask, sp):
    m, s = ALGEBRA_MASKS[mask], SPACINGS[sp]
    r = 1.6 * max(s)
    c, o = DR.margin(m, "close", r, s), DR.margin(m, "open", r, s)
    assert not (m & ~c).any() and not (o & ~m).any()
    assert np.array_equal(DR.margin(c, "close", r, s), c) and np.array_equal(DR.margin(o, "open", r, s), o)
    assert (c ^ m).any() or (o ^ m).any()
    full, none = np.ones_like(m), np.zeros_like(m)
    for op in DR.OPS:
        assert DR.margin(full, op, r, s).all() and not DR.margin(none, op, r, s).any()
    band = np.random.default_rng(1).random(m.shape) < 0.5
    g = DR.margin(m, "grow", r, s, band=band)
    assert not (m & ~g).any() and not (g & ~m & ~band).any() and (g & ~m).any()


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxDistanceParams, VxDistanceResult, VxMarginParams
    for cls, names, want in (
            (VxDistanceParams, ["spacing", "max_distance", "side"], [20, 0, 12, 16]),
            (VxDistanceResult, ["finite", "max_d2", "argmax"], [24, 0, 8, 12]),
            (VxMarginParams, ["op", "radius", "spacing", "band"], [24, 0, 4, 8, 20])):
        assert cls is getattr(_abi, cls.__name__)
        assert [f[0] for f in cls._fields_] == names
        got = offsets(tmp_path, cls.__name__, names)
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n in names] == want


def test_enums_match_the_header():
    from volxel_amd import _abi
    from volxel_amd.renderer import Volxel3DRenderer
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    for name, value in _abi.MARGIN_OPS.items():
        assert int(re.search(r"VX_MARGIN_%s = (\d+)" % name.upper(), text).group(1)) == value
    for name, value in _abi.DISTANCE_SIDES.items():
        assert int(re.search(r"VX_DISTANCE_%s = (\d+)" % name.upper(), text).group(1)) == value
    assert Volxel3DRenderer.MARGIN_OPS == tuple(sorted(_abi.MARGIN_OPS, key=_abi.MARGIN_OPS.get)) == DR.OPS
    assert Volxel3DRenderer.DISTANCE_SIDES == tuple(sorted(_abi.DISTANCE_SIDES, key=_abi.DISTANCE_SIDES.get))


ENTRY_POINTS = ("vx_segment_distance", "vx_distance_read", "vx_segment_margin", "vx_distance_stats")


def test_entry_points_are_declared_exported_and_bound_in_both_hosts(native_lib):
    from volxel_amd import _abi
    napi = os.path.join(ROOT, "volxel_amd", "napi")
    c = open(os.path.join(napi, "volxel_napi_distance.c")).read()      # the addon of the distance calls
    js = open(os.path.join(napi, "viewer.js")).read()
    dts = open(os.path.join(napi, "index.d.ts")).read()
    for name in ENTRY_POINTS:
        assert name in _abi.declared_symbols("volxel_hip.h")
        assert getattr(native_lib, name).argtypes is not None              # bound with a signature by load_library
        assert name + "(" in c
    for m in ("segmentMargin(", "segmentDistance(", "distanceStats("):
        assert m in js and m in dts
    for word in DR.OPS + ("outside", "inside"):
        assert f"'{word}'" in js and f"'{word}'" in dts


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_distance_addon_boundary(tmp_path):
    """volxel_napi_distance.node: its exported names and its argument-count and handle guards; no device is touched: every
    call here is refused before the C ABI is reached.  volxel_napi.node keeps the exports it had."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "volxel_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    arity = {"segmentMargin": 7, "segmentDistance": 6, "distanceRead": 2, "distanceStats": 1}
    script = r"""
const path = require('path');
const native = require(path.join(process.argv[2], 'volxel_napi_distance.node'));
const arity = JSON.parse(process.argv[3]);
const thrown = (f) => { try { f(); return null; } catch (e) { return { type: e instanceof TypeError, msg: e.message }; } };
const out = { keys: Object.keys(native).sort(), none: {}, short: {}, handle: {},
              main: Object.keys(require(path.join(process.argv[2], 'volxel_napi.node'))) };
for (const k of out.keys) {
  out.none[k] = thrown(() => native[k]());
  out.short[k] = thrown(() => native[k](...new Array(arity[k] - 1).fill({})));   // one argument too few
  out.handle[k] = thrown(() => native[k]({}, ...new Array(arity[k] - 1).fill(0)));
}
console.log(JSON.stringify(out));
"""
    (tmp_path / "b.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "b.js"), NAPI, json.dumps(arity)], timeout=120))
    assert out["keys"] == sorted(arity) and not set(arity) & set(out["main"])
    for k in arity:
        for kind in ("none", "short"):
            e = out[kind][k]
            assert e is not None and e["type"] and "wrong number of arguments" in e["msg"], (k, kind, e)
        e = out["handle"][k]
        assert e is not None and e["type"] and "expected a context handle" in e["msg"], (k, e)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    invalid = int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))
    d, m = _abi.VxDistanceParams(), _abi.VxMarginParams()
    buf = np.zeros(8, dtype=np.float32)
    assert native_lib.vx_segment_distance(None, C.byref(d), None) == invalid
    assert native_lib.vx_distance_read(None, buf.ctypes.data, 8) == invalid
    assert native_lib.vx_segment_margin(None, C.byref(m), None) == invalid
    assert native_lib.vx_distance_stats(None, None, None) == invalid


@pytest.mark.parametrize("kw, word", [
    (dict(op="dilate", radius=1.0), "op"), (dict(op=0, radius=1.0), "op"), (dict(op="grow", radius=0), "radius"),
    (dict(op="grow", radius=-2.0), "radius"), (dict(op="shrink", radius=float("inf")), "radius"),
    (dict(op="open", radius=float("nan")), "radius"), (dict(op="close", radius="3"), "radius"),
    (dict(op="close", radius=True), "radius"),
    (dict(op="grow", radius=1.0, spacing=(1.0, 1.0)), "spacing"), (dict(op="grow", radius=1.0, spacing=(1.0, 0.0, 1.0)), "spacing"),
    (dict(op="grow", radius=1.0, spacing=(1.0, -1.0, 1.0)), "spacing"),
    (dict(op="grow", radius=1.0, spacing=(1.0, float("nan"), 1.0)), "spacing"),
    (dict(op="grow", radius=1.0, spacing=(1.0, float("inf"), 1.0)), "spacing"), (dict(op="grow", radius=1.0, spacing=2.0), "spacing"),
    (dict(op="grow", radius=1.0, band=1), "band"), (dict(op="shrink", radius=1.0, band=True), "band"),
    (dict(op="close", radius=1.0, band=True), "band"),
])
def test_python_refusals_of_segment_margin(kw, word):
    with pytest.raises(ValueError, match=word):
        renderer_shell().segment_margin(**kw)


@pytest.mark.parametrize("kw, word", [
    (dict(side="both"), "side"), (dict(side=1), "side"), (dict(max_distance=0.0), "max_distance"),
    (dict(max_distance=-1.0), "max_distance"), (dict(max_distance=float("nan")), "max_distance"),
    (dict(max_distance=-float("inf")), "max_distance"), (dict(max_distance=None), "max_distance"),
    (dict(spacing=(0.5, 0.5)), "spacing"), (dict(spacing=(0.5, 0.5, 0.0)), "spacing"),
])
def test_python_refusals_of_segment_distance(kw, word):
    with pytest.raises(ValueError, match=word):
        renderer_shell().segment_distance(**kw)


def test_no_volume_is_refused_by_name():
    from volxel_amd import VolxelError
    r = renderer_shell()
    r.volume = None
    for call, name in ((lambda: r.segment_margin("grow", 1.0), "segment_margin"), (lambda: r.segment_distance(), "segment_distance"),
                       (lambda: r.distance_field(), "distance_field")):
        with pytest.raises(VolxelError, match=name):
            call()


def test_default_spacing_is_the_column_norms_of_the_grid_transform():
    from volxel_amd import _checks
    t = np.eye(4)
    t[:3, :3] = np.array([[0.0, -0.5, 0.0], [0.7, 0.0, 0.0], [0.0, 0.0, 2.5]])    # a rotated scan: columns of length 0.7, 0.5, 2.5
    t[:3, 3] = (10.0, -3.0, 7.0)
    assert _checks.spacing(None, t) == tuple(float(F32(v)) for v in (0.7, 0.5, 2.5))
    assert _checks.spacing(None, np.eye(4)) == (1.0, 1.0, 1.0)
    assert _checks.spacing((0.5, 0.5, 2), t) == (0.5, 0.5, 2.0)
    assert _checks.spacing(np.array([0.1, 0.2, 0.3]), t) == tuple(float(F32(v)) for v in (0.1, 0.2, 0.3))
    assert _checks.distance("radius", 5, allow_inf=False) == 5.0 and _checks.distance("max_distance", np.inf, allow_inf=True) == np.inf
    assert _checks.distance("radius", 0.1, allow_inf=False) == float(F32(0.1))
    # the preprocessor's grid of a stack with spacing (0.5, 0.5, 0.8): the spacing comes back
    from volxel_amd import read_u16_stack_to_grid
    from volxel_amd.scene import from_flat
    g = read_u16_stack_to_grid(np.arange(512, dtype=np.uint16).reshape(8, 8, 8), (0.5, 0.5, 0.8))
    assert np.allclose(_checks.spacing(None, from_flat(g.transform)), (0.5, 0.5, 0.8), rtol=1e-6)
