"""Segment views on the GPU (vx_set_segment_view, DESIGN.md section 2 "Segment views").

Restatement-free pins: a volume A+B whose blobs lie in disjoint bricks with an empty brick between them; ONLY(segment of A) and
HIDE(segment of B) must equal the UNMASKED render of a volume holding A alone, bit for bit -- every covered mode, jitter on,
launches of 1, 3 and 32 frames, the isosurface image, hits, counters and pick -- on brickf32, bricku8 and AUTO.  HIDE of an empty
segment and ONLY of the whole volume equal the plain render; ONLY of an empty segment equals the render of a volume that is 0
inside the clip box.
Against the restatement (tests/segview_ref.py) on value noise with a ragged band segment (6- and 26-connected): MIP / MinIP and
the isosurface bit for bit, DVR within the deterministic-DVR tolerance (2e-6).  Then the refusals, the state rules, slices left
alone and the JS host."""
import json
import shutil

import numpy as np
import pytest

from tests import common
from tests import segview_ref as SV
from tests.common import F32_MAX, bits, frame, grid, renderer, small_noise
from tests.js_host import dump_grid, run_node

W, H = 96, 64
LAYOUTS = {k: common.LAYOUTS[k] for k in ("brickf32", "bricku8", "auto")}
MODES = ("dvr", "dvr_phong", "mip", "minip")
# sample_range: every density of both blobs is in range, B shows unless a view hides it
SETTINGS = dict(dvr_step_voxels=0.5, dvr_jitter=False, max_samples=1 << 20, sample_range=(0.0, 1.0))


@pytest.fixture(scope="module")
def scenes():
    ab, a, _ = SV.blobs()
    # the background: no voxel inside CLIP_BACK (a volume must have one voxel above 0; this one, at the far corner, is clipped away
    # and shares A+B's largest value)
    zero = np.zeros_like(ab)
    zero[63, 63, 63] = ab.max()
    return {"ab": grid(ab), "a": grid(a), "zero": grid(zero), "noise": grid(*small_noise(64)), "ab_raw": ab, "a_raw": a}


CLIP_BACK = (40.0 / 64.0, 1.0, 1.0)   # volume_clip_max that leaves brick columns x 5 .. 7 out


def _scene(g, mode, layout=None, jitter=False, devices=None, **kw):
    return renderer(g, layout, devices, mode, (W, H), **{**SETTINGS, "dvr_jitter": jitter}, **kw)


def _seed_of(raw, xlo, xhi):
    """the voxel (x, y, z) of the largest value in x range [xlo, xhi)"""
    sub = np.where((np.arange(raw.shape[2]) >= xlo) & (np.arange(raw.shape[2]) < xhi), raw, 0)
    z, y, x = np.unravel_index(int(np.argmax(sub)), raw.shape)
    return int(x), int(y), int(z)


def _segment_blob(r, raw, xlo, xhi):
    """the segment of the ball in x range [xlo, xhi): every voxel above 0 there (26-connected: the ball is solid)"""
    s = r.segment(_seed_of(raw, xlo, xhi), 1e-30, connectivity=26)
    want = (raw > 0) & (np.arange(raw.shape[2]) >= xlo) & (np.arange(raw.shape[2]) < xhi)
    assert np.array_equal(r.segment_mask(), want)
    return s


def _iso(r):
    rgba, hit = r.isosurface(0.3, skip=True)
    return rgba, hit, r.iso_stats()[:5]


# ---- restatement-free pins ----------------------------------------------------------------------------------------------------

@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
def test_two_blobs_equal_a_alone(scenes, layout, mode):
    ab = scenes["ab_raw"]
    plain = _scene(scenes["a"], mode, layout=LAYOUTS[layout], jitter=True)
    masked = _scene(scenes["ab"], mode, layout=LAYOUTS[layout], jitter=True)
    try:
        want = {n: frame(plain, n, in_flight=32)[0] for n in (1, 3, 32)}
        assert float(want[32][..., :3].max()) > 0.0
        for view, (xlo, xhi) in (("only", (0, 24)), ("hide", (32, 64))):
            _segment_blob(masked, ab, xlo, xhi)
            masked.segment_view = view
            for n in (1, 3, 32):
                got = frame(masked, n, in_flight=32)[0]
                assert np.array_equal(bits(got), bits(want[n])), (view, n, float(np.abs(got - want[n]).max()))
        masked.segment_view = "off"
        if mode != "minip":   # (MinIP is TF(0) on every ray of this scene: the blobs are surrounded by zeros)
            assert not np.array_equal(frame(masked, 1)[0], want[1])   # B is visible again
    finally:
        plain.close()
        masked.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_two_blobs_isosurface_and_pick(scenes, layout):
    ab = scenes["ab_raw"]
    plain = _scene(scenes["a"], "dvr", layout=LAYOUTS[layout])
    masked = _scene(scenes["ab"], "dvr", layout=LAYOUTS[layout])
    try:
        w_rgba, w_hit, w_counts = _iso(plain)
        assert w_counts[1] > 0 and w_counts[4] > 0   # hits; range skipping passed samples over in the plain volume
        picks = [(x, y) for x in range(4, W, 11) for y in range(3, H, 7)]
        w_pick = [plain.pick(x, y, 0.3) for x, y in picks]
        for view, (xlo, xhi) in (("only", (0, 24)), ("hide", (32, 64))):
            _segment_blob(masked, ab, xlo, xhi)
            masked.segment_view = view
            rgba, hit, counts = _iso(masked)
            assert np.array_equal(bits(rgba), bits(w_rgba)) and np.array_equal(bits(hit), bits(w_hit)), view
            # no range skipping under a view: every sample the plain launch passed over is evaluated
            assert counts[4] == 0 and counts[:2] + counts[3:4] == w_counts[:2] + w_counts[3:4], (counts, w_counts)
            assert counts[2] == w_counts[2] + w_counts[4], (counts, w_counts)
            assert [masked.pick(x, y, 0.3) for x, y in picks] == w_pick
    finally:
        plain.close()
        masked.close()


@pytest.mark.gpu
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
@pytest.mark.parametrize("mode", MODES)
def test_empty_and_whole_segments(scenes, layout, mode):
    ab = scenes["ab_raw"]
    r = _scene(scenes["ab"], mode, layout=LAYOUTS[layout], jitter=True, volume_clip_max=CLIP_BACK)
    z = _scene(scenes["zero"], mode, layout=LAYOUTS[layout], jitter=True, volume_clip_max=CLIP_BACK)
    try:
        plain = frame(r, 3, in_flight=32)[0]
        background = frame(z, 3, in_flight=32)[0]
        if mode != "minip":   # (MinIP of A+B meets a zero on every ray: it is the background too)
            assert not np.array_equal(plain, background)
        s = r.segment(_seed_of(ab, 0, 64), 1e30)              # lo above every density: empty
        assert s.count == 0
        r.segment_view = "hide"
        assert np.array_equal(bits(frame(r, 3, in_flight=32)[0]), bits(plain))
        r.segment_view = "only"
        assert np.array_equal(bits(frame(r, 3, in_flight=32)[0]), bits(background))
        s = r.segment((0, 0, 0), -F32_MAX)                    # every voxel: the whole volume
        assert s.count == ab.size
        assert np.array_equal(bits(frame(r, 3, in_flight=32)[0]), bits(plain))
        r.segment_view = "hide"
        assert np.array_equal(bits(frame(r, 3, in_flight=32)[0]), bits(background))
    finally:
        r.close()
        z.close()


# ---- against the restatement --------------------------------------------------------------------------------------------------

def _band(r, g, conn):
    """a ragged segment of the noise volume: the density band [q0.6, q0.95] grown from its largest voxel"""
    from tests import segment_ref as SG
    p = r.bind_uniforms()
    d = SG.densities(g, p.volume_density_scale, p.volume_inv_maj)
    lo, hi = float(np.quantile(d, 0.6)), float(np.quantile(d, 0.95))
    pred = SG.predicate(d, lo, hi)
    z, y, x = np.unravel_index(int(np.argmax(np.where(pred, d, -np.inf))), d.shape)
    r.segment((int(x), int(y), int(z)), lo, hi, connectivity=conn)
    m = r.segment_mask()
    assert 0 < m.sum() < m.size
    return m


@pytest.mark.gpu
@pytest.mark.parametrize("conn", (6, 26))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_device_matches_restatement(scenes, layout, conn):
    g = scenes["noise"]
    r = _scene(g, "mip", layout=LAYOUTS[layout], dvr_skip_empty=True, use_env=False, show_environment=False)
    try:
        m = _band(r, g, conn)
        for view in SV.VIEWS:
            r.segment_view = view
            for mode in ("mip", "minip"):
                r.settings.render_mode = mode
                img = frame(r)[0]
                c = r.counters()
                tf, L = r._tf
                want, n, ntf, rays = SV.projection_image(r._params, g, tf, L, m, view, minip=mode == "minip")
                assert np.array_equal(img, want), (view, mode, float(np.abs(img - want).max()))
                assert c.samples == n and c.skip_steps == 0 and c.tf_samples == ntf and c.rays == rays
            r.settings.render_mode = "dvr"
            img = frame(r)[0]
            tf, L = r._tf
            want, _ = SV.dvr_image(r._params, g, tf, L, m, view)
            assert np.abs(img - want).max() <= 2e-6, (view, float(np.abs(img - want).max()))
            rgba, hit = r.isosurface(0.45, skip=True)
            counts = r.iso_stats()[:5]
            w_rgba, w_hit, wc, _ = SV.isosurface(r._params, g, 0.45, m, view)
            assert np.array_equal(bits(hit), bits(w_hit)), view
            assert counts == (wc["rays"], wc["hits"], wc["samples"], wc["refine_samples"], 0), (counts, wc)
            assert np.abs(rgba - w_rgba).max() <= 1e-5
    finally:
        r.close()


# ---- refusals and state -------------------------------------------------------------------------------------------------------

def _refused(fn, *words):
    from volxel_amd import VolxelError
    with pytest.raises(VolxelError) as e:
        fn()
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.gpu
def test_refusals(scenes):
    ab = scenes["ab_raw"]
    r = _scene(scenes["ab"], "dvr")
    try:
        assert r.segment_view == "off"

        def setv(v):
            r.segment_view = v
        _refused(lambda: setv("only"), "without a current segment")
        _refused(lambda: setv("sideways"), "segment_view must be one of")
        rc = r._lib.vx_set_segment_view(r._ctx, 3)
        assert rc != 0 and b"is not VX_SEGVIEW_OFF" in r._lib.vx_last_error(r._ctx)
        _segment_blob(r, ab, 0, 24)
        r.segment_view = "hide"
        frame(r)
        for mode in ("default", "no_dda", "raymarch"):
            r.settings.render_mode = mode
            _refused(lambda: frame(r), "path-traced render mode")
        r.settings.render_mode = "dvr"
        r.settings.debug_hits = True
        _refused(lambda: frame(r), "debug_hits")
        r.settings.debug_hits = False
        r.settings.use_env = False
        r.settings.dvr_shadow_stride = 2
        _refused(lambda: frame(r), "shadowed DVR")
        r.settings.dvr_shadow_stride = 0
        r.settings.dvr_ert_epsilon = 1.0
        _refused(lambda: frame(r), "no LDS-window kernel")
        r.settings.dvr_ert_epsilon = 1e-4
        for lay in (0, 1):   # reference, cellquad
            r.set_layout(lay)
            _refused(lambda: frame(r), "no LDS-window kernel")
        r.set_layout(2)
        frame(r)
        _iso(r)
        # an upload drops the segment and resets the view: renders go on
        r.setup_from_grid(scenes["ab"])
        assert r.segment_view == "off"
        frame(r)
        _refused(lambda: setv("hide"), "without a current segment")
    finally:
        r.close()
    g = _scene(scenes["ab"], "dvr", devices=[0, 0])
    try:
        g.segment(_seed_of(ab, 0, 24), 1e-30, connectivity=26)
        _refused(lambda: setattr(g, "segment_view", "only"), "device group")
        assert g.segment_view == "off"
    finally:
        g.close()


@pytest.mark.gpu
def test_new_segment_changes_image_and_slices_stay(scenes):
    from volxel_amd import mpr
    ab = scenes["ab_raw"]
    r = _scene(scenes["ab"], "mip")
    try:
        sp = mpr.axial(r, 12)
        sl_plain = r.slice(sp)
        _segment_blob(r, ab, 0, 24)
        r.segment_view = "hide"
        hide_a = frame(r)[0]
        assert np.array_equal(r.slice(sp), sl_plain)           # slices keep the unmasked data
        _segment_blob(r, ab, 32, 64)
        assert r.frame_index == 0                              # segment() restarted accumulation under a view
        hide_b = frame(r)[0]
        assert not np.array_equal(hide_a, hide_b)
        assert np.array_equal(r.slice(sp), sl_plain)
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_js_host_segment_view_has_the_python_bits(scenes, tmp_path):
    ab = scenes["ab_raw"]
    g = scenes["ab"]
    seed = _seed_of(ab, 32, 64)
    r = _scene(g, "dvr")
    try:
        r.segment(seed, 1e-30, connectivity=26)
        r.segment_view = "hide"
        r.render(frames=4)
        want = r.read_accum()
        # the native calls no other JS-host test reaches, on one shadowed frame: setLayout, readShadowGrid, shadowStats,
        # readDisplayScaled, readDisplay and resetCounters must answer what these answer
        r.setup_from_grid(g)
        r.set_layout(2)
        r.settings.use_env = r.settings.show_environment = False
        r.settings.dvr_shadow_stride = 2
        r.restart_rendering()
        r.render(frames=1)
        light, (builds, light_samples, _) = r.read_shadow_grid(), r.shadow_stats()
        scaled, full = r.read_display(), np.empty((H, W, 4), dtype=np.uint8)
        r._check(r._lib.vx_read_display(r._ctx, full.ctypes.data, float(r.settings.exposure), float(r.settings.gamma)))
        r.reset_counters()
        extra = {"dims": list(light.shape[::-1]), "builds": builds, "lightSamples": light_samples,
                 "samplesAfterReset": r.counters().samples}
    finally:
        r.close()
    dump_grid(tmp_path, g)
    (tmp_path / "args.json").write_text(json.dumps({"seed": list(seed)}))
    body = r"""
const a = JSON.parse(fs.readFileSync(path.join(dir, 'args.json')));
r.settings.dvrStepVoxels = 0.5;
r.settings.dvrJitter = false;
r.settings.maxSamples = 1 << 20;
r.settings.sampleRange = [0, 1];
const before = r.segmentView;
let refused = false;
try { r.segmentView = 'only'; } catch (e) { refused = /without a current segment/.test(e.message); }
r.segment(a.seed, 1e-30, { connectivity: 26 });
r.segmentView = 'hide';
r.render(4);
const img = r.readAccum();
fs.writeFileSync(path.join(dir, 'img.bin'), Buffer.from(img.buffer, img.byteOffset, img.byteLength));
const view = r.segmentView;
r.setupFromGrid(grid);
v.native.setLayout(r.ctx, 2);
r.settings.useEnv = r.settings.showEnvironment = false;
r.settings.dvrShadowStride = 2;
r.restartRendering();
r.render(1);
const light = r.readShadowGrid(), ss = r.shadowStats(), full = new Uint8Array(r.width * r.height * 4);
v.native.readDisplay(r.ctx, full, r.settings.exposure, r.settings.gamma);
save('light.bin', light.data); save('scaled.bin', r.readDisplay()); save('full.bin', full);
r.resetCounters();
const extra = { dims: light.dims, builds: ss.builds, lightSamples: ss.lightSamples, samplesAfterReset: r.counters().samples };
fs.writeFileSync(path.join(dir, 'extra.json'), JSON.stringify(extra));
console.log(JSON.stringify({ before, refused, view, after: r.segmentView }));
r.dispose();
"""
    out = run_node(tmp_path, body, size=(W, H))
    assert out == {"before": "off", "refused": True, "view": "hide", "after": "off"}, out
    got = np.fromfile(tmp_path / "img.bin", dtype=np.float32).reshape(want.shape)
    assert np.array_equal(bits(got), bits(want))
    assert json.loads((tmp_path / "extra.json").read_text()) == extra and extra["builds"] == 1 and extra["samplesAfterReset"] == 0
    assert np.array_equal(np.fromfile(tmp_path / "light.bin", dtype=np.float32), light.ravel())
    assert np.array_equal(np.fromfile(tmp_path / "scaled.bin", dtype=np.uint8), scaled.ravel()) and scaled.any()
    assert np.array_equal(np.fromfile(tmp_path / "full.bin", dtype=np.uint8), full.ravel())
