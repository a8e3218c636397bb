"""Slices without a GPU (vx_slice, DESIGN.md section 2 "Slices"): the ABI of the entry points and of VxSliceParams, the planes of
volxel_amd.mpr, the refusals of the Python host, the NumPy restatement (tests/slice_ref.py) against closed forms, and the Node
host carrying the new calls."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import types

import numpy as np
import pytest

from oracle import np_oracle as NP
from tests import slice_ref as SR

from tests.common import NAPI, ROOT
F32 = np.float32


@pytest.fixture(scope="module")
def noise():
    from tests.common import small_noise
    from volxel_amd import read_u16_stack_to_grid
    return read_u16_stack_to_grid(*small_noise(32))


def _stub(grid):
    """what mpr.oblique reads of a renderer: its current params"""
    from tests.common import make_scene
    _, _, vol, _, p = make_scene(grid, 16, 16, "dvr")
    return types.SimpleNamespace(_params=p, volume=vol)


def test_entry_points_are_declared_and_exported(native_lib):
    from volxel_amd import _abi
    for name in ("vx_slice", "vx_slice_stats"):
        assert name in _abi.declared_symbols("volxel_hip.h")
        getattr(native_lib, name)


def test_slice_params_parse():
    from volxel_amd import _abi, VxSliceParams
    assert VxSliceParams is _abi.VxSliceParams
    names = [f[0] for f in VxSliceParams._fields_]
    assert names == ["origin", "du", "dv", "dn", "size", "slab_samples", "reduce", "display", "window"]
    assert C.sizeof(VxSliceParams) == 4 * (12 + 2 + 1 + 1 + 1 + 2)
    assert VxSliceParams.size.offset == 48 and VxSliceParams.window.offset == 68
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    for name, value in (("VX_SLICE_MEAN", _abi.SLICE_MEAN), ("VX_SLICE_MAX", _abi.SLICE_MAX), ("VX_SLICE_MIN", _abi.SLICE_MIN),
                        ("VX_SLICE_NONE", _abi.SLICE_NONE), ("VX_SLICE_GREY", _abi.SLICE_GREY), ("VX_SLICE_TF", _abi.SLICE_TF)):
        assert int(re.search(r"%s\s*=\s*(\d+)" % name, text).group(1)) == value


def _vec(sp, name):
    return list(getattr(sp, name)[:])


def test_index_planes(noise):
    from volxel_amd import axial, coronal, sagittal
    e = [int(x) for x in noise.index_extent]
    a, c, s = axial(noise, 5), coronal(noise, 6), sagittal(noise, 7)
    assert (_vec(a, "origin"), _vec(a, "du"), _vec(a, "dv"), _vec(a, "dn"), list(a.size)) == \
        ([0, 0, 5], [1, 0, 0], [0, 1, 0], [0, 0, 1], [e[0], e[1]])
    assert (_vec(c, "origin"), _vec(c, "du"), _vec(c, "dv"), _vec(c, "dn"), list(c.size)) == \
        ([0, 6, 0], [1, 0, 0], [0, 0, 1], [0, 1, 0], [e[0], e[2]])
    assert (_vec(s, "origin"), _vec(s, "du"), _vec(s, "dv"), _vec(s, "dn"), list(s.size)) == \
        ([7, 0, 0], [0, 1, 0], [0, 0, 1], [1, 0, 0], [e[1], e[2]])
    for sp in (a, c, s):
        assert sp.slab_samples == 1 and sp.reduce == 0 and sp.display == 0
    for bad in (-1, e[2], 2.5):
        with pytest.raises(ValueError):
            axial(noise, bad)
    assert list(axial(_stub(noise), 3).size) == [e[0], e[1]]       # a renderer's volume serves as well


def _centre_world(p, q):
    """world position of cell-frame position q (index q + 1/2) through density_transform"""
    m = np.asarray(p.density_transform[:], dtype=np.float64).reshape(4, 4).T
    return (m @ np.append(np.asarray(q, dtype=np.float64) + 0.5, 1.0))[:3]


def test_oblique_along_index_z_reproduces_axial(noise):
    from volxel_amd import axial, oblique
    r = _stub(noise)
    p = r._params
    e = [int(x) for x in noise.index_extent]
    k = 11
    vox = float(np.asarray(p.density_transform[:], dtype=np.float64)[0])      # world size of one voxel along x
    c = _centre_world(p, [(e[0] - 1) / 2, (e[1] - 1) / 2, k])
    ob = oblique(r, center=c, normal=(0, 0, 1), up=(0, 1, 0), pixel_size=vox, size=(e[0], e[1]))
    ax = axial(noise, k)
    for name in ("origin", "du", "dv", "dn"):
        if name == "dn":
            assert _vec(ob, name) == [0, 0, 0]       # thickness 0
            continue
        assert np.allclose(_vec(ob, name), _vec(ax, name), rtol=0, atol=1e-5 * max(e)), name
    assert list(ob.size) == list(ax.size) and ob.slab_samples == 1


def test_oblique_slab_spacing_and_anisotropy():
    from tests.common import small_noise
    from volxel_amd import oblique, read_u16_stack_to_grid
    v, _ = small_noise(32)
    g = read_u16_stack_to_grid(v, (0.5, 1.0, 2.0))
    r = _stub(g)
    p = r._params
    m = np.asarray(p.density_transform[:], dtype=np.float64).reshape(4, 4).T
    sx, sy, sz = m[0, 0], m[1, 1], m[2, 2]         # world units per index unit along each axis
    assert sx < sy < sz
    c = _centre_world(p, [10, 10, 10])
    sp = oblique(r, center=c, normal=(0, 0, 1), up=(0, 1, 0), pixel_size=0.01, size=(9, 5), thickness=0.08, samples=4)
    assert np.allclose(_vec(sp, "du"), [0.01 / sx, 0, 0], rtol=1e-6, atol=1e-7)
    assert np.allclose(_vec(sp, "dv"), [0, 0.01 / sy, 0], rtol=1e-6, atol=1e-7)
    assert np.allclose(_vec(sp, "dn"), [0, 0, 0.02 / sz], rtol=1e-6, atol=1e-7)
    # centred: pixel ((W-1)/2, (H-1)/2) at slab position (N-1)/2 is the centre
    mid = np.asarray(_vec(sp, "origin")) + 4 * np.asarray(_vec(sp, "du")) + 2 * np.asarray(_vec(sp, "dv")) + \
        1.5 * np.asarray(_vec(sp, "dn"))
    assert np.allclose(mid, [10, 10, 10], atol=1e-4)
    for kw in (dict(normal=(0, 0, 0)), dict(up=(0, 0, 2)), dict(pixel_size=0.0), dict(samples=0), dict(samples=4097),
               dict(size=(0, 4)), dict(size=(16385, 4)), dict(thickness=-1.0), dict(center=(np.nan, 0, 0))):
        args = dict(center=c, normal=(0, 0, 1), up=(0, 1, 0), pixel_size=0.01, size=(9, 5))
        args.update(kw)
        with pytest.raises(ValueError):
            oblique(r, **args)


def test_python_refusals(noise):
    from volxel_amd import Volxel3DRenderer, axial
    r = object.__new__(Volxel3DRenderer)      # the checks come before any library call
    r._ctx = None
    sp = axial(noise, 0)
    with pytest.raises(TypeError):
        r.slice("plane")
    with pytest.raises(ValueError):
        r.slice(sp, reduce="median")
    with pytest.raises(ValueError):
        r.slice(sp, display="rgb")
    for window in (None, (1.0, 1.0), (0.5, 0.2), (0.0, float("inf")), (0.0,)):
        with pytest.raises(ValueError):
            r.slice(sp, display="grey", window=window)
    with pytest.raises(ValueError):
        r.slice(sp, display="tf", window=(0.0, 1.0))
    for field, value in (("size", (0, 4)), ("size", (4, 16385)), ("slab_samples", 0), ("slab_samples", 4097)):
        q = type(sp).from_buffer_copy(sp)
        if field == "size":
            q.size[0], q.size[1] = value
        else:
            setattr(q, field, value)
        with pytest.raises(ValueError):
            r.slice(q)
    q = type(sp).from_buffer_copy(sp)
    q.du[1] = float("nan")
    with pytest.raises(ValueError):
        r.slice(q)


def test_reference_axial_is_the_voxels(noise):
    from volxel_amd import axial
    p = _stub(noise)._params
    vol = NP.NpVolume(noise)
    e = [int(x) for x in noise.index_extent]
    x, y = np.meshgrid(np.arange(e[0]), np.arange(e[1]))
    for k in (0, 9, e[2] - 1):
        got = SR.values(axial(noise, k), noise, p)
        want = (F32(p.volume_density_scale) * vol.brick(x, y, np.full_like(x, k))) * F32(p.volume_inv_maj)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert float(want.max()) >= 0


def test_reference_axis_slab_is_the_max_and_min_of_its_slices(noise):
    """an axis-aligned slab with integer origin and dn = (0, 0, 1) takes exact positions: its MAX / MIN are the element-wise
    max / min of the N axial slices it covers"""
    from volxel_amd import axial
    p = _stub(noise)._params
    k0, n = 4, 6
    sp = axial(noise, k0)
    sp.slab_samples = n
    slices = np.stack([SR.values(axial(noise, k0 + s), noise, p) for s in range(n)])
    assert np.array_equal(SR.values(sp, noise, p, reduce=SR.MAX), slices.max(axis=0))
    assert np.array_equal(SR.values(sp, noise, p, reduce=SR.MIN), slices.min(axis=0))
    mean = SR.values(sp, noise, p, reduce=SR.MEAN)
    acc = slices[0]
    for s in range(1, n):
        acc = acc + slices[s]
    assert np.array_equal(mean, acc / F32(n))
    assert not np.array_equal(slices.max(axis=0), slices.min(axis=0))
    # N = 1 mean, and max / min over N copies of one position, are the thin slice
    thin = slices[0]
    one = axial(noise, k0)
    assert np.array_equal(SR.values(one, noise, p, reduce=SR.MEAN), thin)
    still = axial(noise, k0)
    still.slab_samples = 5
    still.dn[2] = 0.0
    for red in (SR.MAX, SR.MIN):
        assert np.array_equal(SR.values(still, noise, p, reduce=red), thin)


def test_reference_displays():
    sp = types.SimpleNamespace(window=[F32(0.25), F32(0.75)], display=SR.GREY)
    v = np.array([-1.0, 0.25, 0.5, 0.75, 2.0, 0.2500001], dtype=F32)
    g = SR.display(v, sp)
    assert g[:, 0].tolist() == [0, 0, 128, 255, 255, 0] and (g[:, 3] == 255).all()
    assert (g[:, 0] == g[:, 1]).all() and (g[:, 1] == g[:, 2]).all()
    tf = np.array([[1.0, 0.5, 0.0, 0.5], [0.0, 1.0, 1.0, 1.0]], dtype=F32)
    t = SR.display(np.array([0.1, 0.9, 1.5], dtype=F32), types.SimpleNamespace(display=SR.TF), tf, 2, (0.0, 1.0))
    assert t.tolist() == [[128, 64, 0, 255], [0, 255, 255, 255], [0, 0, 0, 255]]


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_module_exposes_the_slice(native_lib, tmp_path):
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = r"""
const v = require(process.argv[2]);
console.log(JSON.stringify({ methods: Object.getOwnPropertyNames(v.Volxel3DDicomRenderer.prototype),
  natives: [typeof v.native.slice, typeof v.native.sliceStats], size: v.native.sizeofSliceParams() }));
"""
    (tmp_path / "m.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "m.js"), NAPI], timeout=120))
    from volxel_amd import _abi
    for m in ("slice", "sliceStats", "axial", "coronal", "sagittal"):
        assert m in out["methods"]
    assert out["natives"] == ["function", "function"] and out["size"] == C.sizeof(_abi.VxSliceParams)
    dts = open(os.path.join(NAPI, "index.d.ts")).read()
    assert "slice(spec: SliceSpec" in dts and "sliceStats()" in dts
