"""Slices and thick slabs on the GPU (vx_slice, DESIGN.md section 2 "Slices"): the index-space planes against the decoded voxels,
oblique thin and thick slabs of every reduction under every layout against the NumPy restatement (tests/slice_ref.py) with
tolerance 0, both displays, the stats, rendering left alone, device groups, the refusals, a full-size slab and the JS host."""
import ctypes as C
import json
import shutil

import numpy as np
import pytest

from oracle import np_oracle as NP
from tests import slice_ref as SR
from tests.common import F32, LAYOUTS, bits, grid, renderer, small_noise, upload_volume
from tests.js_host import dump_grid, run_node

REDUCE = ("mean", "max", "min")


@pytest.fixture(scope="module")
def noise():
    return grid(*small_noise(64))


@pytest.fixture(scope="module")
def aniso():
    """48 x 40 x 32 voxels of noise with spacing (0.8, 1.0, 2.5): the world box is not a cube"""
    v, _ = small_noise(64, seed=3)
    return grid(np.ascontiguousarray(v[:32, :40, :48]), (0.8, 1.0, 2.5))


def _tilted(r, thickness=0.0, samples=1, size=(80, 72)):
    """an oblique plane through the volume, tilted about two axes; its corners lie outside the volume"""
    from volxel_amd import oblique
    return oblique(r, center=(0.05, -0.04, 0.02), normal=(0.3, -0.5, 0.8), up=(0.1, 1.0, 0.2), pixel_size=0.016, size=size,
                   thickness=thickness, samples=samples)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_axis_planes_are_the_voxels(noise, layout):
    """closed form: at voxel centres every fraction is 0, so the value is the decoded voxel x density_scale x inv_maj"""
    from volxel_amd import axial, coronal, sagittal
    r = renderer(noise, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        got = {(f.__name__, i): r.slice(f(r, i)) for f in (axial, coronal, sagittal) for i in (0, 17, 63)}
        p = r._params
    finally:
        r.close()
    vol = NP.NpVolume(noise)
    n = 64
    a, b = np.meshgrid(np.arange(n), np.arange(n))       # a = pixel x, b = pixel y

    def want(x, y, z):
        return (F32(p.volume_density_scale) * vol.brick(x, y, z)) * F32(p.volume_inv_maj)

    for (name, i), v in got.items():
        assert v.shape == (n, n)
        if name == "axial":
            w = want(a, b, np.full_like(a, i))
        elif name == "coronal":
            w = want(a, np.full_like(a, i), b)
        else:
            w = want(np.full_like(a, i), a, b)
        assert np.array_equal(bits(v), bits(w)), (name, i)
    assert any(float(v.max()) > 0 for v in got.values())


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["brickf32", "bricku8", "reference", "cellquad"])
@pytest.mark.parametrize("reduce", REDUCE)
@pytest.mark.parametrize("thick", [False, True])
def test_oblique_matches_reference(noise, layout, reduce, thick):
    r = renderer(noise, layout=LAYOUTS[layout], dvr_jitter=False)
    try:
        sp = _tilted(r, thickness=0.12, samples=9) if thick else _tilted(r)
        got = r.slice(sp, reduce=reduce)
        want = SR.values(sp, noise, r._params, reduce=SR.REDUCE_IDS[reduce])
    finally:
        r.close()
    assert np.array_equal(bits(got), bits(want)), float(np.abs(got - want).max())
    assert (got == 0).any() and float(got.max()) > 0       # part of the plane lies outside the volume


@pytest.mark.gpu
def test_anisotropic_oblique_matches_reference(aniso):
    r = renderer(aniso, dvr_jitter=False)
    try:
        sp = _tilted(r, thickness=0.05, samples=4, size=(33, 47))
        got = r.slice(sp, reduce="max")
        want = SR.values(sp, aniso, r._params, reduce=SR.MAX)
    finally:
        r.close()
    assert np.array_equal(bits(got), bits(want))
    assert float(got.max()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("display", ["grey", "tf"])
def test_display_bytes(noise, display):
    r = renderer(noise, dvr_jitter=False)
    try:
        sp = _tilted(r, thickness=0.1, samples=5)
        window = (0.05, 0.6) if display == "grey" else None
        vals, rgba = r.slice(sp, reduce="max", display=display, window=window)
        tf, L = r._tf
        q = type(sp).from_buffer_copy(sp)
        q.display = SR.GREY if display == "grey" else SR.TF
        if window:
            q.window[0], q.window[1] = window
        want = SR.display(vals, q, tf, L, r._params.sample_range[:])
    finally:
        r.close()
    assert rgba.shape == vals.shape + (4,) and rgba.dtype == np.uint8
    assert np.array_equal(rgba, want)
    assert (rgba[..., 3] == 255).all() and int(rgba[..., :3].max()) > 0


@pytest.mark.gpu
def test_stats_count_the_samples(noise):
    r = renderer(noise, dvr_jitter=False)
    try:
        assert r.slice_stats() == (0, 0.0)
        sp = _tilted(r, thickness=0.1, samples=7, size=(50, 30))
        r.slice(sp)
        n, ms = r.slice_stats()
        lib, ctx = r._lib, r._ctx
        assert lib.vx_slice(ctx, C.byref(sp), None, None) == 0      # the kernel alone
        n2, _ = r.slice_stats()
    finally:
        r.close()
    assert n == n2 == 50 * 30 * 7 and ms > 0.0


@pytest.mark.gpu
def test_slicing_leaves_rendering_alone(noise):
    from volxel_amd import axial

    def run(with_slice):
        r = renderer(noise, dvr_jitter=False)
        try:
            r.reset_counters()
            r.render(frames=4, in_flight=4)
            if with_slice:
                r.slice(_tilted(r, thickness=0.1, samples=3), reduce="min", display="tf")
                r.slice(axial(r, 5))
            r.render(frames=4, in_flight=4)
            img, c = r.read_accum(), r.counters()
        finally:
            r.close()
        return img, (c.samples, c.rays, c.pixels, c.frames, c.launches)

    a, ca = run(False)
    b, cb = run(True)
    assert np.array_equal(bits(a), bits(b))
    assert ca == cb and ca[0] > 0


@pytest.mark.gpu
def test_group_gives_the_single_context_bits(noise):
    one = renderer(noise, dvr_jitter=False)
    grp = renderer(noise, devices=[0, 0, 0], dvr_jitter=False)
    try:
        sp = _tilted(one, thickness=0.1, samples=6)
        a, ra = one.slice(sp, reduce="max", display="tf")
        b, rb = grp.slice(sp, reduce="max", display="tf")
        sa, sb = one.slice_stats()[0], grp.slice_stats()[0]
    finally:
        one.close()
        grp.close()
    assert np.array_equal(bits(a), bits(b)) and np.array_equal(ra, rb) and sa == sb


@pytest.mark.gpu
def test_refusals(noise):
    from volxel_amd import _abi, axial
    lib = _abi.load_library()
    sp = axial(noise, 3)
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.vx_slice(ctx, C.byref(sp), None, None) == 3                      # VX_ERR_NO_VOLUME
        assert lib.vx_slice_stats(ctx, None, None) == 0
        assert upload_volume(lib, ctx, noise) == 0
        assert lib.vx_slice(ctx, C.byref(sp), None, None) == 1 and b"vx_set_params" in lib.vx_last_error(ctx)
        r = renderer(noise, dvr_jitter=False)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_resize(ctx, 64, 48) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        assert lib.vx_slice(ctx, C.byref(sp), None, None) == 0
        q = _abi.VxSliceParams.from_buffer_copy(sp)
        q.display = _abi.SLICE_TF
        assert lib.vx_slice(ctx, C.byref(q), None, None) == 1 and b"transfer function" in lib.vx_last_error(ctx)
        assert lib.vx_slice(ctx, None, None, None) == 1 and b"sp" in lib.vx_last_error(ctx)

        def refused(field, value, word):
            q = _abi.VxSliceParams.from_buffer_copy(sp)
            if isinstance(field, tuple):
                getattr(q, field[0])[field[1]] = value
            else:
                setattr(q, field, value)
            if field == ("window", 1) or field == ("window", 0):
                q.display = _abi.SLICE_GREY
            assert lib.vx_slice(ctx, C.byref(q), None, None) == 1, (field, value)
            assert word in lib.vx_last_error(ctx), (field, lib.vx_last_error(ctx))

        refused(("size", 0), 0, b"size[0]")
        refused(("size", 1), 16385, b"size[1]")
        refused("slab_samples", 0, b"slab_samples")
        refused("slab_samples", 4097, b"slab_samples")
        refused("reduce", 3, b"reduce")
        refused("reduce", -1, b"reduce")
        refused("display", 3, b"display")
        for name in ("origin", "du", "dv", "dn"):
            refused((name, 1), float("nan"), name.encode())
            refused((name, 2), float("inf"), name.encode())
        refused(("window", 1), 0.0, b"window")                   # window[1] == window[0]
        refused(("window", 1), -1.0, b"window")
        refused(("window", 0), float("nan"), b"window")
        vals = np.empty(64 * 64, dtype=np.float32)
        rgba = np.empty(64 * 64 * 4, dtype=np.uint8)
        assert lib.vx_slice(ctx, C.byref(sp), vals.ctypes.data, rgba.ctypes.data) == 1 and b"rgba8_out" in lib.vx_last_error(ctx)
    finally:
        lib.vx_destroy(ctx)


@pytest.mark.gpu
def test_full_size_mip_slab():
    """a 1024^2 oblique 64-sample MIP slab of the 512^3 config-3 volume, against slice_ref on a 96 x 64 crop"""
    from volxel_amd import synth
    g = grid(*synth.value_noise(512))
    r = renderer(g, dvr_jitter=False)
    try:
        sp = _tilted(r, thickness=0.06, samples=64, size=(1024, 1024))
        vals, rgba = r.slice(sp, reduce="max", display="tf")
        n, _ = r.slice_stats()
        win = (464, 480, 560, 544)
        want = SR.values(sp, g, r._params, reduce=SR.MAX, window=win)
    finally:
        r.close()
    x0, y0, x1, y1 = win
    assert n == 1024 * 1024 * 64
    assert np.array_equal(bits(vals[y0:y1, x0:x1]), bits(want))
    assert float(want.max()) > 0


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_slice_has_the_python_bits(noise, tmp_path):
    dims = [int(x) for x in noise.index_extent]
    r = renderer(noise, dvr_jitter=False)
    try:
        from volxel_amd import axial
        sp = _tilted(r, thickness=0.1, samples=5)
        want_v, want_rgba = r.slice(sp, reduce="min", display="grey", window=(0.0, 0.5))
        want_ax = r.slice(axial(r, 9))
    finally:
        r.close()
    spec = {k: [float(x) for x in getattr(sp, k)[:]] for k in ("origin", "du", "dv", "dn")}
    spec.update(size=[int(sp.size[0]), int(sp.size[1])], slabSamples=int(sp.slab_samples))
    (tmp_path / "spec.json").write_text(json.dumps(spec))
    dump_grid(tmp_path, noise)
    body = r"""
const spec = JSON.parse(fs.readFileSync(path.join(dir, 'spec.json')));
const a = r.slice(Object.assign({}, spec, { reduce: 'min', display: 'grey', window: [0.0, 0.5] }));
const b = r.slice(r.axial(9));
fs.writeFileSync(path.join(dir, 'js_v.bin'), Buffer.from(a.values.buffer));
fs.writeFileSync(path.join(dir, 'js_rgba.bin'), Buffer.from(a.rgba8.buffer));
fs.writeFileSync(path.join(dir, 'js_ax.bin'), Buffer.from(b.values.buffer));
console.log(JSON.stringify({ samples: r.sliceStats().samples, axNull: b.rgba8 === null }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert out["axNull"] and out["samples"] == dims[0] * dims[1]
    assert np.array_equal(np.fromfile(tmp_path / "js_v.bin", dtype=np.uint32), bits(want_v).reshape(-1))
    assert np.array_equal(np.fromfile(tmp_path / "js_rgba.bin", dtype=np.uint8), want_rgba.reshape(-1))
    assert np.array_equal(np.fromfile(tmp_path / "js_ax.bin", dtype=np.uint32), bits(want_ax).reshape(-1))
