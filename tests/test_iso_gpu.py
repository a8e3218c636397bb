"""First-hit isosurfaces on the GPU (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): every layout with range skipping off and on
against the NumPy restatement (tests/iso_ref.py) -- hit buffer and counters bit for bit, colour within Phong's 1e-5 --, windows
and picking against the full image, the float64 pins of tests/test_iso_host.py on the device, rendering left alone, device
groups, the refusals, the JS host and config 2 (the CT phantom at 1080p) at a bone threshold."""
import ctypes as C
import shutil

import numpy as np
import pytest

from tests import iso_ref as IR
from tests.common import F32, LAYOUTS, bits, grid, renderer, small_noise, upload_volume
from tests.js_host import dump_grid, run_node
from tests.shapes import ISO_CASES, ISO_COLOUR, ISO_PHONG, SPACINGS, Field, iso_params

COLOUR = (0.9, 0.6, 0.4)
PHONG = (0.2, 0.6, 0.5, 24.0)
W, H = 64, 48


@pytest.fixture(scope="module")
def noise():
    return grid(*small_noise(64))


@pytest.fixture(scope="module")
def phantom():
    """config 2's CT phantom at 64^3: air around the body, where range skipping passes samples over"""
    from volxel_amd import synth
    return grid(*synth.ct_phantom(64))


def _renderer(g, layout=None, devices=None, mode="dvr"):
    return renderer(g, layout, devices, mode, (W, H), dvr_jitter=False, volume_clip_min=(0.1, 0.0, 0.05),
                    volume_clip_max=(0.9, 0.85, 1.0))


def _stats(r):
    rays, hits, samples, refine, skipped, _ = r.iso_stats()
    return {"rays": rays, "hits": hits, "samples": samples, "refine_samples": refine, "skipped": skipped}


def _check(r, g, iso, skip, refine=8, window=None, lib=None):
    rgba, hit = r.isosurface(iso, color=COLOUR, phong=PHONG, refine=refine, skip=skip, window=window)
    st = _stats(r)
    p = r._params
    bound = IR.bound_table(lib, g, p) if skip else None
    want_rgba, want_hit, want_counts, per = IR.isosurface(p, g, iso, color=COLOUR, phong=PHONG, refine=refine, window=window,
                                                          bound=bound)
    assert np.array_equal(bits(hit), bits(want_hit))
    assert st == want_counts, (st, want_counts)
    assert float(np.abs(rgba - want_rgba).max()) <= 1e-5
    return rgba, hit, st, per


@pytest.mark.gpu
@pytest.mark.parametrize("volume", ["noise", "phantom"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("skip", [False, True])
def test_device_matches_reference(request, volume, layout, skip):
    """DVR's rays and samples, the first hit, the bisection, t and w bit for bit; counters exact (the skipped samples are the
    bound table's); colour within 1e-5.  dvr_jitter and the render mode have no effect"""
    from volxel_amd import _abi
    lib = _abi.load_library()
    g = request.getfixturevalue(volume)
    r = _renderer(g, layout=LAYOUTS[layout], mode="mip" if layout == "auto" else "dvr")
    try:
        r.settings.dvr_jitter = True
        refined = skipped = 0
        isos = ((0.35, 8), (0.6, 3), (0.05, 0)) if volume == "noise" else ((0.3, 8), (0.75, 3), (0.05, 0))
        for iso, refine in isos:
            _, hit, st, per = _check(r, g, iso, skip, refine=refine, lib=lib)
            assert st["hits"] > 50, (iso, st)
            refined += int((per["found"] & ~per["cap"]).sum())
            skipped += st["skipped"]
        assert refined > 50
        if skip and volume == "phantom":
            assert skipped > 0
    finally:
        r.close()


@pytest.mark.gpu
def test_skipping_gives_the_same_bits(noise):
    r = _renderer(noise)
    try:
        for iso in (0.3, 0.55, 0.8):
            a_rgba, a_hit = r.isosurface(iso, skip=False)
            sa = _stats(r)
            b_rgba, b_hit = r.isosurface(iso, skip=True)
            sb = _stats(r)
            assert np.array_equal(bits(a_hit), bits(b_hit)) and np.array_equal(bits(a_rgba), bits(b_rgba))
            assert sa["samples"] + sa["skipped"] == sb["samples"] + sb["skipped"] and sa["skipped"] == 0
            assert (sa["rays"], sa["hits"], sa["refine_samples"]) == (sb["rays"], sb["hits"], sb["refine_samples"])
    finally:
        r.close()


@pytest.mark.gpu
def test_window_and_pick_reproduce_the_image(noise):
    r = _renderer(noise)
    try:
        rgba, hit = r.isosurface(0.4, refine=16)
        full = _stats(r)
        win = (5, 7, 45, 30)
        wr, wh = r.isosurface(0.4, refine=16, window=win)
        x0, y0, x1, y1 = win
        assert wr.shape == (y1 - y0, x1 - x0, 4)
        assert np.array_equal(bits(wr), bits(rgba[y0:y1, x0:x1])) and np.array_equal(bits(wh), bits(hit[y0:y1, x0:x1]))
        assert _stats(r)["rays"] < full["rays"]
        f = hit[..., 3] >= 0
        ys, xs = np.nonzero(f)
        for i in np.linspace(0, len(xs) - 1, 6).astype(int):
            pt = r.pick(int(xs[i]), int(ys[i]), 0.4)
            assert pt is not None and np.array_equal(np.asarray(pt, F32).view(np.uint32), bits(hit[ys[i], xs[i], :3]))
        ym, xm = np.nonzero(~f)
        assert len(xm) and r.pick(int(xm[0]), int(ym[0]), 0.4) is None
    finally:
        r.close()


def _raw(r, p, iso, refine, skip, color=ISO_COLOUR, phong=ISO_PHONG):
    from volxel_amd import _abi
    q = _abi.VxIsoParams()
    q.iso = iso
    q.color[0], q.color[1], q.color[2] = color
    q.ka, q.kd, q.ks, q.shininess = phong
    q.refine, q.skip = refine, int(skip)
    w, h = int(p.res[0]), int(p.res[1])
    rgba = np.empty((h, w, 4), dtype=F32)
    hit = np.empty((h, w, 4), dtype=F32)
    r._check(r._lib.vx_isosurface(r._ctx, C.byref(q), rgba.ctypes.data, hit.ctypes.data))
    return rgba, hit


@pytest.fixture(scope="module")
def fields():
    from oracle import oracle as O
    return {(k, sp): Field(O, k, SPACINGS[sp]) for k in ("flat", "ramp", "bowl") for sp in SPACINGS}


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(ISO_CASES))
def test_device_meets_the_float64_pins(fields, name):
    """the cases of tests/test_iso_host.py on layouts 0, 1, 2 and 4, skipping off and on: the device's hit buffer is the
    restatement's bit for bit, so it meets the tier-2 and tier-1 bounds the host file holds the restatement to"""
    from volxel_amd import Volxel3DRenderer
    case = ISO_CASES[name]
    fd = fields[case.kind, case.spacing]
    p = iso_params(case, fd)
    want_rgba, want_hit, counts, per = IR.isosurface(p, fd.grid, case.iso, color=ISO_COLOUR, phong=case.phong, refine=case.refine)
    for layout in (0, 1, 2, 4):
        for skip in (False, True):
            r = Volxel3DRenderer(int(p.res[0]), int(p.res[1]), layout=layout)
            try:
                r.setup_from_grid(fd.grid)
                r._check(r._lib.vx_set_params(r._ctx, C.byref(p)))
                rgba, hit = _raw(r, p, case.iso, case.refine, skip, phong=case.phong)
                st = _stats(r)
            finally:
                r.close()
            assert np.array_equal(bits(hit), bits(want_hit)), (layout, skip)
            assert float(np.abs(rgba - want_rgba).max()) <= 1e-5, (layout, skip)
            assert st["hits"] == counts["hits"] and st["samples"] + st["skipped"] == counts["samples"]


@pytest.mark.gpu
def test_isosurface_leaves_rendering_alone(noise):
    def run(with_iso):
        r = _renderer(noise)
        try:
            r.reset_counters()
            r.render(frames=4, in_flight=4)
            if with_iso:
                r.isosurface(0.4)
                r.isosurface(0.6, skip=False, window=(3, 4, 20, 30))
                r.pick(30, 20, 0.5)
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
    one = _renderer(noise)
    grp = _renderer(noise, devices=[0, 0, 0])
    try:
        a = one.isosurface(0.45, color=COLOUR, phong=PHONG)
        sa = _stats(one)
        b = grp.isosurface(0.45, color=COLOUR, phong=PHONG)
        sb = _stats(grp)
    finally:
        one.close()
        grp.close()
    assert np.array_equal(bits(a[0]), bits(b[0])) and np.array_equal(bits(a[1]), bits(b[1])) and sa == sb


@pytest.mark.gpu
def test_refusals(noise):
    from volxel_amd import _abi
    lib = _abi.load_library()
    q = _abi.VxIsoParams()
    q.iso, q.refine, q.skip = 0.5, 4, 1
    ctx = C.c_void_p()
    assert lib.vx_create(0, C.byref(ctx)) == 0
    try:
        assert lib.vx_isosurface(ctx, C.byref(q), None, None) == 3                    # VX_ERR_NO_VOLUME
        assert lib.vx_iso_stats(ctx, None, None, None, None, None, None) == 0
        assert upload_volume(lib, ctx, noise) == 0
        assert lib.vx_isosurface(ctx, C.byref(q), None, None) == 1 and b"vx_set_params" in lib.vx_last_error(ctx)
        r = _renderer(noise)
        try:
            p = r.bind_uniforms()
        finally:
            r.close()
        assert lib.vx_resize(ctx, W, H) == 0 and lib.vx_set_params(ctx, C.byref(p)) == 0
        assert lib.vx_isosurface(ctx, C.byref(q), None, None) == 0
        assert lib.vx_isosurface(ctx, None, None, None) == 1 and b"ip" in lib.vx_last_error(ctx)

        def refused(field, value, word):
            b = _abi.VxIsoParams.from_buffer_copy(q)
            if isinstance(field, tuple):
                getattr(b, field[0])[field[1]] = value
            else:
                setattr(b, field, value)
            assert lib.vx_isosurface(ctx, C.byref(b), None, None) == 1, (field, value)
            assert word in lib.vx_last_error(ctx), (field, lib.vx_last_error(ctx))

        for name in ("iso", "ka", "kd", "ks", "shininess"):
            refused(name, float("nan"), name.encode())
            refused(name, float("inf"), name.encode())
        refused(("color", 1), float("nan"), b"color[1]")
        refused("shininess", -1.0, b"shininess")
        refused("refine", 17, b"refine")
        refused("skip", 2, b"skip")
        refused("skip", -1, b"skip")
        for win in ((0, 0, 0, 4), (5, 0, 5, 4), (0, 0, W + 1, 4), (0, 0, 4, H + 1), (0, 10, 4, 3)):
            b = _abi.VxIsoParams.from_buffer_copy(q)
            b.window[0], b.window[1], b.window[2], b.window[3] = win
            assert lib.vx_isosurface(ctx, C.byref(b), None, None) == 1 and b"window" in lib.vx_last_error(ctx), win
    finally:
        lib.vx_destroy(ctx)


@pytest.mark.gpu
def test_config2_bone_at_1080p():
    """config 2 (the 256^3 CT phantom, spacing (0.7, 0.7, 1.0)) at 1920 x 1080 at a bone threshold: a 96 x 64 crop of the full
    image, centred on the bone, against the restatement, bit for bit"""
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, synth
    g = grid(*synth.ct_phantom(256))
    r = Volxel3DRenderer(1920, 1080, device=0)
    try:
        r.setup_from_grid(g)
        r.restore_settings(BENCHMARK_SETTINGS)
        r.settings.volume_clip_min, r.settings.volume_clip_max = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
        r.settings.dvr_step_voxels = 0.5
        iso = 0.75
        rgba, hit = r.isosurface(iso, refine=8)
        st = _stats(r)
        # a 96 x 64 crop centred on the bone's image (the centroid of the hit pixels)
        ys, xs = np.nonzero(hit[..., 3] >= 0)
        assert len(xs) > 10000
        cx, cy = int(np.clip(np.median(xs), 48, 1920 - 48)), int(np.clip(np.median(ys), 32, 1080 - 32))
        win = (cx - 48, cy - 32, cx + 48, cy + 32)
        want_rgba, want_hit, _, per = IR.isosurface(r._params, g, iso, refine=8, window=win,
                                                    phong=tuple(r.settings.phong))
    finally:
        r.close()
    x0, y0, x1, y1 = win
    assert np.array_equal(bits(hit[y0:y1, x0:x1]), bits(want_hit))
    assert float(np.abs(rgba[y0:y1, x0:x1] - want_rgba).max()) <= 1e-5
    assert per["found"].sum() > 100 and st["hits"] == len(xs)


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_isosurface_has_the_python_bits(noise, tmp_path):
    r = _renderer(noise)
    try:
        want_rgba, want_hit = r.isosurface(0.4, color=COLOUR, phong=PHONG, refine=6)
        want_st = _stats(r)
        win_rgba, win_hit = r.isosurface(0.4, window=(4, 6, 30, 20))
        pt = r.pick(32, 24, 0.4)
    finally:
        r.close()
    dump_grid(tmp_path, noise)
    body = r"""
r.settings.volumeClipMin = [0.1, 0.0, 0.05]; r.settings.volumeClipMax = [0.9, 0.85, 1.0];
const a = r.isosurface(0.4, { color: [0.9, 0.6, 0.4], phong: [0.2, 0.6, 0.5, 24.0], refine: 6 });
const st = r.isoStats();
const w = r.isosurface(0.4, { window: [4, 6, 30, 20] });
const pt = r.pick(32, 24, 0.4);
fs.writeFileSync(path.join(dir, 'rgba.bin'), Buffer.from(a.rgba.buffer));
fs.writeFileSync(path.join(dir, 'hit.bin'), Buffer.from(a.hit.buffer));
fs.writeFileSync(path.join(dir, 'wrgba.bin'), Buffer.from(w.rgba.buffer));
fs.writeFileSync(path.join(dir, 'whit.bin'), Buffer.from(w.hit.buffer));
console.log(JSON.stringify({ st, size: [a.width, a.height, w.width, w.height], pt: pt === null ? null : Array.from(new Float32Array(pt)) }));
r.dispose();
"""
    out = run_node(tmp_path, body)
    assert out["size"] == [64, 48, 26, 14]
    assert np.array_equal(np.fromfile(tmp_path / "rgba.bin", dtype=np.uint32), bits(want_rgba).reshape(-1))
    assert np.array_equal(np.fromfile(tmp_path / "hit.bin", dtype=np.uint32), bits(want_hit).reshape(-1))
    assert np.array_equal(np.fromfile(tmp_path / "wrgba.bin", dtype=np.uint32), bits(win_rgba).reshape(-1))
    assert np.array_equal(np.fromfile(tmp_path / "whit.bin", dtype=np.uint32), bits(win_hit).reshape(-1))
    st = out["st"]
    assert [st[k] for k in ("rays", "hits", "samples", "refineSamples", "skipped")] == \
        [want_st[k] for k in ("rays", "hits", "samples", "refine_samples", "skipped")]
    assert (pt is None) == (out["pt"] is None)
    if pt is not None:
        assert np.array_equal(np.asarray(out["pt"], F32), np.asarray(pt, F32))
