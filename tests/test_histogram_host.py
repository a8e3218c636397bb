"""The histograms without a device (DESIGN.md section 2 "Histograms"): the restatement (tests/histogram_ref.py) against
np.histogram, np.sort and a brute-force Otsu; and the hosts' plumbing: struct layouts, enums, exports, the addon's boundary,
refusals.  CPU only."""
import ctypes as C
import json
import math
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from tests import histogram_ref as HR
from tests.common import F32, NAPI, ROOT
from tests.shapes import offsets, renderer_shell


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bins", [1, 2, 256, 1024])
def test_linear_rule_is_np_histogram_on_dyadic_densities(bins):
    """densities k / 1024 over (0, 1): every quotient of the rule is exact, so the fp32 rule and NumPy's float64 one must agree
    on every edge, the last included"""
    rng = np.random.default_rng(bins)
    d = (rng.integers(0, 1025, size=20000) / 1024.0).astype(F32)
    d = np.concatenate([d, np.arange(1025, dtype=F32) / F32(1024)])           # every value at least once, 0 and 1 included
    counts, below, above = HR.linear(d, bins, 0.0, 1.0)
    want, _ = np.histogram(d.astype(np.float64), bins=bins, range=(0.0, 1.0))
    assert below == 0 and above == 0 and np.array_equal(counts, want.astype(np.uint64))
    assert counts.dtype == np.uint64 and int(counts.sum()) == d.size


def tricky_values():
    """a few hundred floats with negatives, both zeros, duplicates, denormals and the extremes"""
    rng = np.random.default_rng(11)
    tiny = np.array([1, 2, 3, 0x7fffff], dtype=np.uint32).view(F32)                    # denormals
    parts = [rng.normal(0.0, 1.0, 150).astype(F32), np.zeros(30, F32), -np.zeros(7, F32), tiny, -tiny, np.repeat(F32(0.25), 40),
             np.repeat(F32(-1.5), 9), np.array([np.finfo(F32).max, -np.finfo(F32).max, np.finfo(F32).tiny], dtype=F32),
             (rng.integers(0, 8, 60) / 8.0).astype(F32)]
    d = np.concatenate(parts)
    rng.shuffle(d)
    return d


def test_order_key_is_the_order_of_the_floats():
    d = np.unique(tricky_values())
    k = HR.order_key(d)
    assert np.all(np.diff(k.astype(np.int64)) > 0)                                     # np.unique sorts ascending
    assert HR.order_key(np.array([-0.0], F32))[0] + 1 == HR.order_key(np.array([0.0], F32))[0]
    for x in d:
        assert HR.key_float(HR.order_key(np.array([x], F32))[0]).view(np.uint32) == F32(x).view(np.uint32)


def test_three_pass_select_is_np_sort_at_every_rank():
    d = tricky_values()
    want = np.sort(d)
    # (np.sort leaves the order of -0 and +0 open; the key order puts -0 first)
    exact = d[np.argsort(HR.order_key(d), kind="stable")]
    assert np.array_equal(want, exact)
    for k in range(d.size):
        got = HR.select(d, k)
        assert got == want[k] and got.view(np.uint32) == exact[k].view(np.uint32), k
    # every pass partitions the array
    for prefix, p, b in ((0, 0, 11), (1027, 11, 11), (0x3fffff, 22, 10), (5, 3, 12), (0x7fffffff, 31, 1)):
        c, below, above = HR.key_pass(d, prefix, p, b)
        assert c.size == 1 << b and int(c.sum()) + below + above == d.size


def test_select_inside_a_long_tie():
    d = np.concatenate([np.zeros(30000, F32), np.linspace(-1, 1, 501).astype(F32)])
    want = np.sort(d)
    for k in (0, 249, 250, 251, 15000, 30250, 30251, d.size - 1):
        assert HR.select(d, k) == want[k]
    for q in (0, 25, 50, 75, 100, 33.3):
        assert HR.select(d, HR.lower_rank(q, d.size)) == np.percentile(d, q, method="lower")


RANGES = [(256, 0.0, 1.0), (7, 0.1, 0.9), (4096, 0.0, 1.0), (1, -2.0, 3.0), (100, 0.25, 0.75), (3, 0.5, float(np.nextafter(F32(0.5), F32(1)))),
          (4096, 0.5, float(F32(0.5) + F32(2.0 ** -20)))]


@pytest.mark.parametrize("bins, lo, hi", RANGES)
def test_linear_rule_partitions_and_is_monotone(bins, lo, hi):
    rng = np.random.default_rng(5)
    lo32, hi32 = F32(lo), F32(hi)
    w = float(hi32) - float(lo32)
    near = (float(lo32) + rng.uniform(-0.5, 1.5, 4000) * w).astype(F32)
    # the neighbours of both ends and the ends themselves
    ends = np.array([lo32, hi32, np.nextafter(lo32, F32(-9)), np.nextafter(lo32, F32(9)), np.nextafter(hi32, F32(-9)),
                     np.nextafter(hi32, F32(9))], dtype=F32)
    d = np.concatenate([near, ends, rng.uniform(-3, 4, 2000).astype(F32)])
    counts, below, above = HR.linear(d, bins, lo, hi)
    assert below + above + int(counts.sum()) == d.size
    assert below == int((d < lo32).sum()) and above == int((d > hi32).sum())
    b = HR.linear_bins(d, bins, lo, hi)
    order = np.argsort(d, kind="stable")
    inside = (d[order] >= lo32) & (d[order] <= hi32)
    assert np.all(np.diff(b[order][inside]) >= 0)                                      # bins are monotone in d
    assert b[np.flatnonzero(d == hi32)[0]] == bins - 1 and b[np.flatnonzero(d == lo32)[0]] == 0
    assert np.isfinite(HR.inv_of(bins, lo, hi))


def test_moments_and_mean_std():
    d = tricky_values()[:200].astype(F32) / F32(4)
    d = d[np.isfinite(d) & (np.abs(d) < 100)]
    m = HR.moments(d)
    d64 = d.astype(np.float64)
    mean, std = HR.mean_std(m)
    assert m["count"] == d.size and m["d_min"] == d.min() and m["d_max"] == d.max()
    assert abs(mean - d64.mean()) <= 1e-12 and abs(std - d64.std()) <= 1e-12
    e = HR.moments(np.zeros(0, F32))
    assert e == dict(count=0, d_min=0.0, d_max=0.0, d_sum=0.0, d_sum2=0.0) and all(math.isnan(x) for x in HR.mean_std(e))


def bimodal():
    rng = np.random.default_rng(2)
    d = np.concatenate([rng.normal(0.25, 0.04, 6000), rng.normal(0.7, 0.06, 3000)]).astype(F32)
    return np.clip(d, 0.0, 1.0)


@pytest.mark.parametrize("bins", [2, 16, 256])
def test_otsu_against_a_brute_force_over_all_splits(bins):
    from volxel_amd.renderer_segment import otsu_split
    counts, _, _ = HR.linear(bimodal(), bins, 0.0, 1.0)
    var = HR.otsu_variances(counts, 0.0, 1.0)
    k, t = HR.otsu(counts, 0.0, 1.0)
    assert len(var) == bins - 1 and var[k] == max(var) and all(v < var[k] for v in var[:k])
    assert otsu_split(counts, HR.edges(bins, 0.0, 1.0)) == k
    assert t == HR.edges(bins, 0.0, 1.0)[k + 1]
    if bins >= 16:
        assert 0.25 + 2 * 0.04 < t < 0.7 - 2 * 0.06                                   # between the modes


def test_otsu_ties_go_to_the_lowest_split_and_degenerate_histograms_are_refused():
    from volxel_amd.renderer_segment import otsu_split
    for counts, want in (([5, 0, 0, 5], 0), ([0, 3, 0, 0, 3, 0], 1), ([1, 1], 0), ([4, 0, 4, 0, 0], 0), ([0, 0, 7, 9], 2)):
        e = HR.edges(len(counts), 0.0, 1.0)
        assert HR.otsu(counts)[0] == want == otsu_split(np.array(counts, dtype=np.uint64), e), counts
    for counts in ([0, 0, 0], [0, 9, 0], [3]):
        assert HR.otsu(counts)[0] == -1 == otsu_split(np.array(counts, dtype=np.uint64), HR.edges(len(counts), 0.0, 1.0))


# ---- the boundary ---------------------------------------------------------------------------------------------------------------
def test_struct_layouts_match_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxHistogramParams, VxHistogramResult
    for cls, names, want in (
            (VxHistogramParams, ["source", "slot", "box_lo", "box_hi", "rule", "bins", "lo", "hi", "prefix", "prefix_bits", "key_bits",
                                 "moments"], [64, 0, 4, 8, 20, 32, 36, 40, 44, 48, 52, 56, 60]),
            (VxHistogramResult, ["count", "below", "above", "d_sum", "d_sum2", "d_min", "d_max"], [48, 0, 8, 16, 24, 32, 40, 44])):
        assert cls is getattr(_abi, cls.__name__)
        assert [f[0] for f in cls._fields_] == names
        got = offsets(tmp_path, cls.__name__, names)
        assert got == [C.sizeof(cls)] + [getattr(cls, n).offset for n in names] == want


def test_enums_match_the_header():
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    for name, value in _abi.HIST_SOURCES.items():
        assert int(re.search(r"VX_HIST_%s = (\d+)" % name.upper(), text).group(1)) == value
    assert int(re.search(r"VX_HIST_LINEAR = (\d+)", text).group(1)) == _abi.HIST_LINEAR == 0
    assert int(re.search(r"VX_HIST_KEY = (\d+)", text).group(1)) == _abi.HIST_KEY == 1
    assert int(re.search(r"#define VX_HIST_MAX_BINS (\d+)u", text).group(1)) == _abi.HIST_MAX_BINS == 4096
    assert int(re.search(r"#define VX_HIST_MAX_KEY_BITS (\d+)u", text).group(1)) == _abi.HIST_MAX_KEY_BITS == 12
    from volxel_amd.renderer import Volxel3DRenderer
    assert Volxel3DRenderer.RADIX_PASSES == HR.PASSES and sum(b for _, b in HR.PASSES) == 32
    assert all(b <= _abi.HIST_MAX_KEY_BITS and p == sum(x for _, x in HR.PASSES[:i]) for i, (p, b) in enumerate(HR.PASSES))


ENTRY_POINTS = ("vx_histogram", "vx_histogram_stats")
ADDON = {"histogram": 3, "histogramStats": 1}     # the addon's functions on a context and how many arguments each takes
JS_METHODS = ("histogram", "densityOrderStatistic", "densityPercentile", "otsuThreshold", "histogramStats")
PY_METHODS = ("histogram", "density_order_statistic", "density_percentile", "otsu_threshold", "histogram_stats")


def test_entry_points_are_declared_exported_and_bound_in_both_hosts(native_lib):
    from volxel_amd import _abi, Histogram
    from volxel_amd.renderer import Volxel3DRenderer
    c = open(os.path.join(NAPI, "volxel_napi_histogram.c")).read()
    js = open(os.path.join(NAPI, "viewer.js")).read()
    dts = open(os.path.join(NAPI, "index.d.ts")).read()
    for name in ENTRY_POINTS:
        assert name in _abi.declared_symbols("volxel_hip.h")
        assert getattr(native_lib, name).argtypes is not None              # bound with a signature by load_library
        assert name + "(" in c
    for m in JS_METHODS:
        assert f"  {m}(" in js and f"  {m}(" in dts
    for m in ADDON:
        assert f'"{m}"' in c
    for m in PY_METHODS:
        assert callable(getattr(Volxel3DRenderer, m))
    assert "volxel_napi_histogram.node" in open(os.path.join(NAPI, "Makefile")).read()
    assert [f for f in Histogram.__dataclass_fields__] == ["counts", "edges", "below", "above", "count", "d_min", "d_max", "d_sum",
                                                           "d_sum2", "mean", "std"]
    # the kernels live in a header of the segment unit: no new translation unit
    mk = open(os.path.join(ROOT, "volxel_amd", "csrc", "Makefile")).read()
    assert "UNITS = vx_api vx_api_volume vx_api_view vx_api_segment vx_api_mesh\n" in mk
    unit = open(os.path.join(ROOT, "volxel_amd", "csrc", "vx_api_segment.hip")).read()
    assert '#include "vx_histogram.hpp"' in unit


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_histogram_addon_boundary(tmp_path):
    """volxel_napi_histogram.node: its exported names and its argument-count and handle guards; no device is touched: every
    call here is refused before the C ABI is reached.  The three other addons keep the exports they had."""
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "volxel_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = r"""
const path = require('path');
const native = require(path.join(process.argv[2], 'volxel_napi_histogram.node'));
const arity = JSON.parse(process.argv[3]);
const thrown = (f) => { try { f(); return null; } catch (e) { return { type: e instanceof TypeError, msg: e.message }; } };
const out = { keys: Object.keys(native).sort(), size: native.sizeofHistogramParams(), none: {}, short: {}, handle: {}, others: [] };
for (const f of ['volxel_napi.node', 'volxel_napi_distance.node', 'volxel_napi_segments.node'])
  out.others.push(...Object.keys(require(path.join(process.argv[2], f))));
for (const k of Object.keys(arity)) {
  out.none[k] = thrown(() => native[k]());
  out.short[k] = thrown(() => native[k](...new Array(arity[k] - 1).fill({})));   // one argument too few
  out.handle[k] = thrown(() => native[k]({}, ...new Array(arity[k] - 1).fill(0)));
}
console.log(JSON.stringify(out));
"""
    (tmp_path / "b.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "b.js"), NAPI, json.dumps(ADDON)], timeout=120))
    assert out["keys"] == sorted(list(ADDON) + ["sizeofHistogramParams"]) and out["size"] == 64
    assert not set(out["keys"]) & set(out["others"])
    for k in ADDON:
        for kind in ("none", "short"):
            e = out[kind][k]
            assert e is not None and e["type"] and "wrong number of arguments" in e["msg"], (k, kind, e)
        e = out["handle"][k]
        assert e is not None and e["type"] and "expected a context handle" in e["msg"], (k, e)


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_argument_checks_have_the_python_texts(tmp_path):
    """the checks of viewer.js refuse what _checks.py refuses, with the same words; loaded without a device"""
    from volxel_amd import _checks
    subprocess.check_call(["make", "-C", os.path.join(ROOT, "volxel_amd", "csrc"), "-s"])
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    js = open(os.path.join(NAPI, "viewer.js")).read()
    for text in ("must be 'volume', 'segment' or an integer slot 0 .. ", "bins must be an integer 1 .. ",
                 "range must be (lo, hi), two finite numbers with lo < hi, not ", "ranks: every entry must be an integer 0 .. ",
                 "q must be a number or a sequence of numbers in [0, 100], not ", "the region is empty",
                 "fewer than two non-empty bins"):
        assert text in js, text
    for call, text in ((lambda: _checks.hist_source("slot"), "must be 'volume', 'segment' or an integer slot 0 .. 31"),
                       (lambda: _checks.hist_bins(0), "bins must be an integer 1 .. 4096"),
                       (lambda: _checks.hist_range((1, 1)), "range must be (lo, hi), two finite numbers with lo < hi, not "),
                       (lambda: _checks.ranks([5], 5), "ranks: every entry must be an integer 0 .. 4 (the region has 5 voxels)"),
                       (lambda: _checks.percentiles(101), "q must be a number or a sequence of numbers in [0, 100], not ")):
        with pytest.raises(ValueError) as e:
            call()
        assert text in str(e.value)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    invalid = int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))
    hp, res = _abi.VxHistogramParams(), _abi.VxHistogramResult()
    counts = np.zeros(256, dtype=np.uint64)
    launches, ms = C.c_uint32(), (C.c_double * 2)()
    assert native_lib.vx_histogram(None, C.byref(hp), counts.ctypes.data, 256, C.byref(res)) == invalid
    assert native_lib.vx_histogram(None, None, None, 0, None) == invalid
    assert native_lib.vx_histogram_stats(None, C.byref(launches), ms) == invalid


BAD = [
    (lambda r: r.histogram(bins=0), "bins"), (lambda r: r.histogram(bins=4097), "bins"), (lambda r: r.histogram(bins=2.0), "bins"),
    (lambda r: r.histogram(bins=True), "bins"), (lambda r: r.histogram(range=(1.0, 1.0)), "range"),
    (lambda r: r.histogram(range=(0.5, 0.25)), "range"), (lambda r: r.histogram(range=(0.0, math.inf)), "range"),
    (lambda r: r.histogram(range=(math.nan, 1.0)), "range"), (lambda r: r.histogram(range=0.5), "range"),
    (lambda r: r.histogram(range=(0.0, 0.5, 1.0)), "range"), (lambda r: r.histogram(source="slot"), "source"),
    (lambda r: r.histogram(source=32), "source"), (lambda r: r.histogram(source=-1), "source"),
    (lambda r: r.histogram(source=1.0), "source"), (lambda r: r.histogram(source=None), "source"),
    (lambda r: r.histogram(box=((0, 0, 0), (16, 15, 23))), "box"), (lambda r: r.histogram(box=((4, 0, 0), (3, 15, 23))), "box"),
    (lambda r: r.histogram(box=(0, 0, 0)), "box"),
    (lambda r: r.density_order_statistic([0], source="mask"), "source"), (lambda r: r.density_order_statistic(3), "ranks"),
    (lambda r: r.density_order_statistic([-1]), "ranks"), (lambda r: r.density_order_statistic([0.5]), "ranks"),
    (lambda r: r.density_order_statistic([True]), "ranks"), (lambda r: r.density_order_statistic([0], box=((0, 0, 0), (0, 0, 24))), "box"),
    (lambda r: r.density_percentile(101), "q"), (lambda r: r.density_percentile(-0.5), "q"),
    (lambda r: r.density_percentile([50, "x"]), "q"), (lambda r: r.density_percentile(None), "q"),
    (lambda r: r.density_percentile(True), "q"), (lambda r: r.density_percentile(math.nan), "q"),
    (lambda r: r.density_percentile(50, source=40), "source"),
    (lambda r: r.otsu_threshold(bins=0), "bins"), (lambda r: r.otsu_threshold(range=(1.0, 0.0)), "range"),
    (lambda r: r.otsu_threshold(source="bone"), "source"),
]


@pytest.mark.parametrize("call, word", BAD, ids=[f"{i}-{w}" for i, (_, w) in enumerate(BAD)])
def test_python_refusals_by_argument_name(call, word):
    with pytest.raises(ValueError, match=word):
        call(renderer_shell())


def test_no_volume_is_refused_by_name():
    from volxel_amd import VolxelError
    r = renderer_shell()
    r.volume = None
    for call, name in ((lambda: r.histogram(), "histogram"), (lambda: r.density_order_statistic([0]), "density_order_statistic"),
                       (lambda: r.density_percentile(50), "density_percentile"), (lambda: r.otsu_threshold(), "histogram")):
        with pytest.raises(VolxelError, match=name):
            call()


def test_the_shared_checks_accept_what_is_legal():
    from volxel_amd import _checks
    assert _checks.hist_source("volume") == (0, 0) and _checks.hist_source("segment") == (1, 0)
    assert _checks.hist_source(0) == (2, 0) and _checks.hist_source(np.int64(31)) == (2, 31)
    assert _checks.hist_bins(1) == 1 and _checks.hist_bins(np.int32(4096)) == 4096
    assert _checks.hist_range((0, 1)) == (0.0, 1.0) and _checks.hist_range([np.float32(0.1), 0.5]) == (float(F32(0.1)), 0.5)
    assert _checks.ranks([0, 4], 5) == (0, 4) and _checks.ranks(np.arange(3), 3) == (0, 1, 2) and _checks.ranks([10 ** 12]) == (10 ** 12,)
    assert _checks.percentiles(50) == ((50.0,), True) and _checks.percentiles([0, 100.0]) == ((0.0, 100.0), False)
    assert _checks.percentiles(np.float64(12.5)) == ((12.5,), True)
