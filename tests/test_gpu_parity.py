"""GPU parity tests: the HIP path, called through the C ABI (volxel_amd.Volxel3DRenderer ->
libvolxel_hip.so), against the CPU oracle on identical uniforms / volume / TF.

Tolerances (stated per SURVEY 8(c)/BASELINE: max-abs pixel diff <= 1e-4 on the fp32
accumulation buffer):
  * ray generation, slab test, densities, TF bins, sample counts, termination: bit exact;
  * deterministic DVR images: <= 2e-6 (exp / pow come from different math libraries);
  * stochastic reference modes, per frame: >= 99.9 % of pixels within 1e-4 (a 1-ulp log()
    difference can flip a collision decision; SURVEY hard part 1).
"""
import ctypes as C
import os

import numpy as np
import math

import pytest

pytestmark = pytest.mark.gpu

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _renderer(og, tf, L, p_src, layout):
    from volxel_amd import Volxel3DRenderer, _abi
    r = Volxel3DRenderer(p_src.res[0], p_src.res[1], layout=layout)
    r.setup_from_grid(og)
    r.change_transfer_func(tf, L)
    return r


def _render_with_params(r, p, frame=0, weight=0.0):
    """drive the C ABI directly with a prepared uniform block (same block the oracle gets)"""
    r._check(r._lib.vx_set_params(r._ctx, C.byref(p)))
    r._check(r._lib.vx_render_frame(r._ctx, frame, weight))
    return r.read_accum()


def _oracle_env(oracle, r):
    """the renderer's environment map as the oracle takes it (None: directional light)"""
    e = r.environment
    return oracle.Environment(e.floats, e.width, e.height) if e is not None else None


def test_unorm_table():
    from volxel_amd import Volxel3DRenderer
    r = Volxel3DRenderer(64, 64)
    out = np.zeros(256, dtype=np.float32)
    r._check(r._lib.vx_debug_unorm_table(r._ctx, out.ctypes.data))
    want = np.arange(256, dtype=np.float32) / np.float32(255.0)
    assert np.array_equal(out, want)
    name, cus, mem = r.device_info()
    assert "gfx950" in name and cus == 256


@pytest.mark.parametrize("layout", [0, 1, 2, 4])
@pytest.mark.parametrize("name", ["sphere32_debughits", "sphere32_dvr", "noise32_dvr_clip",
                                  "noise32_dvr_jitter_f3", "noise32_phong", "noise32_phong_jitter_f2",
                                  "sphere32_dvr_ortho", "noise32_dvr_ortho_jitter_f1"])
def test_golden_deterministic(oracle, name, layout):
    from tests.golden.make_golden import build_case
    grid, tf, L, p, frame = build_case(oracle, name)
    want = np.load(os.path.join(GOLD, name + ".npz"))
    r = _renderer(grid, tf, L, p, layout)
    r.reset_counters()
    img = _render_with_params(r, p, frame)
    c = r.counters()
    # Phong: the kernels evaluate the Blinn terms on the hardware's 1-ulp rsq / log2 / exp2 (pow = exp2(n*log2 x),
    # n = 32), the oracle on libm: 1e-5, still ten times inside the 1e-4 budget of BASELINE.md
    tol = 1e-5 if "phong" in name else 2e-6
    err = float(np.abs(img - want["image"]).max())
    assert err <= tol, (name, err)
    assert c.samples == int(want["samples"]) and c.rays == int(want["rays"])
    assert c.pixels == p.res[0] * p.res[1]
    if "phong" in name:
        assert c.grad_samples == int(want["grad_samples"])
    if "debughits" in name:
        hit = want["image"][..., 3] == 1  # all pixels; ray-gen + slab are IEEE-exact:
        box = np.abs(want["image"][..., :3] - 0.01).max(axis=2) > 1e-9
        assert np.array_equal(img[box], want["image"][box])


@pytest.mark.parametrize("layout", [1, 2, 4])
def test_dvr_tuned_kernel_equals_generic(oracle, layout):
    """the tuned kernels (cellquad gather, brickf32 LDS tile) and the generic kernel are the
    same function"""
    from tests.golden.make_golden import build_case
    from volxel_amd import Volxel3DRenderer
    grid, tf, L, p, frame = build_case(oracle, "noise32_dvr_clip")
    r = _renderer(grid, tf, L, p, layout)
    a = _render_with_params(r, p, frame)
    ca = r.counters()
    os.environ["VX_DVR_KERNEL"] = "generic"
    try:
        r2 = _renderer(grid, tf, L, p, layout)
    finally:
        del os.environ["VX_DVR_KERNEL"]
    b = _render_with_params(r2, p, frame)
    cb = r2.counters()
    assert ca.samples == cb.samples and ca.rays == cb.rays
    assert ca.lane_slots >= ca.samples and cb.lane_slots == 0
    assert np.abs(a - b).max() <= 2e-6


@pytest.mark.parametrize("mode", ["dvr", "dvr_phong"])
def test_bricku8_equals_brickf32_bit_for_bit(oracle, mode):
    """VX_LAYOUT_BRICKU8 keeps the atlas codes and decodes them while a window is staged (vx_dvr_lds.hpp, U8): the values
    that reach LDS are brickf32's, so accumulated images and every counter are identical -- multi-frame launches with
    jitter, with and without exact empty-space skipping, on a volume with constant and out-of-atlas bricks"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import synth
    inner, sp = synth.value_noise(64, seed=11, zero_quantile=0.5)
    vox = np.zeros((96, 72, 88), dtype=np.uint16)            # extents that are not multiples of 8: padded bricks
    vox[10:74, 4:68, 12:76] = inner
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    res = {}
    for layout in (2, 4):
        for skip in (0, 1):
            s, cam, vol, ds, p = make_scene(g, 200, 136, mode, dvr_jitter=True, dvr_skip_empty=bool(skip),
                                            sample_range=(0.05645751953125, 1.0), **BENCH_CAM)
            r = _renderer(g, tf, L, p, layout)
            r.settings = s; r.camera = cam
            r.reset_counters()
            r.render(frames=21, in_flight=8)                    # 2 single frames (launch order) + 8 + 8 + 3
            c = r.counters()
            res[(layout, skip)] = (r.read_accum(), c.samples, c.rays, c.tf_samples, c.grad_samples, c.lane_slots)
    for skip in (0, 1):
        a, b = res[(2, skip)], res[(4, skip)]
        assert np.array_equal(a[0], b[0]), (mode, skip)
        assert a[1:] == b[1:], (mode, skip, a[1:], b[1:])


@pytest.mark.parametrize("layout", [0, 1, 2, 4])
@pytest.mark.parametrize("name", ["noise32_raymarch", "noise32_no_dda", "noise32_default",
                                  "noise32_default_b3"])
def test_golden_stochastic_modes(oracle, name, layout):
    from tests.golden.make_golden import build_case
    grid, tf, L, p, frame = build_case(oracle, name)
    want = np.load(os.path.join(GOLD, name + ".npz"))
    r = _renderer(grid, tf, L, p, layout)
    r.reset_counters()
    img = _render_with_params(r, p, frame)
    c = r.counters()
    diff = np.abs(img - want["image"]).max(axis=2)
    frac = (diff <= 1e-4).mean()
    assert frac >= 0.999, (name, frac, diff.max())
    assert abs(int(c.samples) - int(want["samples"])) <= 0.002 * int(want["samples"]) + 64
    assert c.rays == int(want["rays"])


@pytest.mark.parametrize("mode,env", [("default", False), ("no_dda", False), ("raymarch", False), ("default", True)])
def test_converged_mean_matches_oracle(oracle, mode, env):
    """SURVEY.md hard part 1 (iii): besides per-frame agreement the CONVERGED image of a stochastic mode must agree within
    Monte-Carlo bounds.  256 accumulation frames of a 64x48 scene are accumulated by the viewer's running mean on the
    device (fragment.frag:155-158 with the weight of viewer.ts:1356: frames 0-4 carry weight 0, frame f >= 5 is
    blended with w = (f - 5) / (f - 4)) and, frame by frame, by the oracle; per pixel and channel
    |mean_HIP - mean_oracle| <= 3 sigma / sqrt(N) with sigma the standard deviation of the oracle's per-frame values
    (+ 2e-6 where sigma is 0: background and fp32 rounding of the recurrence).  A systematic error of the device path
    -- a biased decision, a wrong weight -- would exceed the bound on many pixels at once; an isolated flipped
    collision decision (a 1-ulp log) moves a pixel by its sample value / N, far inside it."""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer, sample_weight
    vox, sp = small_noise(48, seed=3)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    W, H, N, F0 = 64, 48, 256, 5
    r = Volxel3DRenderer(W, H)
    r.setup_from_grid(g)
    r.change_transfer_func(tf, L)
    r.settings.render_mode, r.settings.bounces = mode, 2
    r.settings.sample_range = (0.05, 1.0)
    r.settings.use_env = env
    r.settings.max_samples = 1 << 20
    r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
    r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
    p = r.bind_uniforms()
    r.restart_rendering(); r.reset_counters()
    r.render(frames=F0 + N, rebind=False, in_flight=16)      # frames 0 .. F0 + N - 1, blended on the device
    got = r.read_accum()
    c = r.counters()
    oenv = _oracle_env(oracle, r) if env else None
    frames = np.empty((N, H, W, 3), dtype=np.float32)
    acc = np.zeros((H, W, 4), dtype=np.float32)
    n_samples = 0
    for f in range(F0 + N):
        img, oc = oracle.render(p, g, tf, L, frame_index=f, env=oenv)
        n_samples += oc.samples
        w = np.float32(sample_weight(f))
        # fragment.frag:158 in fp32, as merge_results applies it: fma(1 - w, result, w * prev)
        acc[..., :3] = ((np.float32(1) - w) * img[..., :3].astype(np.float64) + (w * acc[..., :3]).astype(np.float64)).astype(np.float32)
        acc[..., 3] = 1
        if f >= F0:
            frames[f - F0] = img[..., :3]
    mean64 = frames.astype(np.float64).mean(axis=0)
    sigma = frames.astype(np.float64).std(axis=0)
    bound = 3.0 * sigma / math.sqrt(N) + 2e-6
    # the oracle's own recurrence against the plain mean of its frames: the viewer's weights form a running mean
    assert np.abs(acc[..., :3] - mean64).max() <= 1e-5 * max(1.0, float(mean64.max()))
    err = np.abs(got[..., :3].astype(np.float64) - mean64)
    assert (err <= bound).all(), (mode, env, float((err / bound).max()), int((err > bound).sum()))
    assert float(sigma.max()) > 1e-3                       # the scene is not trivially deterministic
    assert abs(int(c.samples) - n_samples) <= 0.002 * n_samples + 64
    print(f"converged mean {mode} env={env}: max err / bound {(err / bound).max():.3f}, max |err| {err.max():.2e}, "
          f"mean sigma {sigma.mean():.3e}")
    r.close()


# ---- row N3: environment-map lighting (environment.ts, envSetup.frag, environment.glsl) ----------
@pytest.mark.parametrize("mode,bounces", [("default", 1), ("default", 3), ("no_dda", 2), ("raymarch", 1), ("default", 0)])
def test_path_kernel_renders_every_layout_and_launch_size(oracle, mode, bounces):
    """render_generic for the path-traced modes on every layout, with and without the environment map, on a ragged image
    (partial workgroups) and in launches of 1, 1, 3 and 2 frames: every launch renders samples and a finite image."""
    from tests.common import benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer
    vox, sp = small_noise(64, seed=9)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    for layout in (0, 1, 2):
        r = Volxel3DRenderer(200, 136, layout=layout)       # not a multiple of 16: partial workgroups
        r.setup_from_grid(g)
        r.change_transfer_func(tf, L)
        r.settings.render_mode, r.settings.bounces = mode, bounces
        r.settings.sample_range = (0.05, 1.0)
        r.settings.use_env = layout != 1                     # directional light on one layout, the map on the others
        r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
        r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
        r.reset_counters()
        r.render(frames=7, in_flight=3)                      # frames 0..6: launches of 1, 1, 3 and 2 frames
        c = r.counters()
        accum, samples = r.read_accum(), c.samples
        r.close()
        assert samples > 0 and np.isfinite(accum).all(), (mode, bounces, layout)


def test_transfer_function_must_be_finite():
    """vx_upload_transfer refuses Inf / NaN entries (the DVR composite is straight-line: 0 * Inf would reach lanes that
    never sampled the entry); the previous table stays in use"""
    from volxel_amd import Volxel3DRenderer, VolxelError
    r = Volxel3DRenderer(64, 64)
    tf = np.ones((16, 4), dtype=np.float32)
    r.change_transfer_func(tf, 16)
    for bad in (np.inf, -np.inf, np.nan):
        t2 = tf.copy()
        t2[5, 2] = bad
        with pytest.raises(VolxelError, match="not finite"):
            r.change_transfer_func(t2, 16)
    r.close()


def test_importance_pyramid_is_bit_identical(oracle):
    """vx_upload_environment builds the 512^2 importance map + mips on the device: same bits as the
    oracle for the default checkerboard and for a random HDR-like map"""
    from volxel_amd import Environment, Volxel3DRenderer
    r = Volxel3DRenderer(64, 64)
    rng = np.random.default_rng(11)
    hdr = np.exp(rng.normal(0, 1.5, size=(37, 64, 4))).astype(np.float32)
    for env in (Environment.default(), Environment(hdr, 64, 37)):
        r.set_environment(env)
        got = np.zeros(oracle.IMP_FLOATS, dtype=np.float32)
        r._check(r._lib.vx_debug_read_importance(r._ctx, got.ctypes.data))
        want = oracle.Environment(env.floats, env.width, env.height).importance
        assert np.array_equal(got, want)
    r.set_environment(None)
    assert r._lib.vx_debug_read_importance(r._ctx, got.ctypes.data) != 0


@pytest.mark.parametrize("name", ["sphere32_debughits_env", "noise32_dvr_env"])
def test_golden_environment_deterministic(oracle, name):
    """background through lookup_environment's map branch; atan/acos come from two math libraries,
    which moves the bilinear weights by ~1e-7 * width: tolerance 1e-5 (2e-6 without a map)"""
    from tests.golden.make_golden import build_case
    grid, tf, L, p, frame = build_case(oracle, name)
    assert p.use_env == 1
    want = np.load(os.path.join(GOLD, name + ".npz"))
    for layout in (0, 1, 2, 4):
        r = _renderer(grid, tf, L, p, layout)
        r.reset_counters()
        img = _render_with_params(r, p, frame)
        c = r.counters()
        assert np.abs(img - want["image"]).max() <= 1e-5, (name, layout)
        assert c.samples == int(want["samples"]) and c.rays == int(want["rays"])


@pytest.mark.parametrize("name", ["noise32_raymarch_env", "noise32_no_dda_env", "noise32_default_b3_env"])
def test_golden_environment_stochastic_modes(oracle, name):
    """light sampling by the hierarchical warp, MIS against pdf_environment, escaped paths"""
    from tests.golden.make_golden import build_case
    grid, tf, L, p, frame = build_case(oracle, name)
    assert p.use_env == 1
    want = np.load(os.path.join(GOLD, name + ".npz"))
    r = _renderer(grid, tf, L, p, 1)
    r.reset_counters()
    img = _render_with_params(r, p, frame)
    c = r.counters()
    diff = np.abs(img - want["image"]).max(axis=2)
    frac = (diff <= 1e-4).mean()
    assert frac >= 0.999, (name, frac, diff.max())
    assert abs(int(c.samples) - int(want["samples"])) <= 0.002 * int(want["samples"]) + 64
    assert c.rays == int(want["rays"])


def test_environment_custom_map_and_errors(oracle):
    """a non-default map, strength from the settings, use_env without a map is refused"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import Environment, synth
    vox, sp = synth.value_noise(32, seed=5, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    rng = np.random.default_rng(5)
    hdr = np.exp(rng.normal(0, 1.0, size=(16, 32, 4))).astype(np.float32)
    env = Environment(hdr, 32, 16, strength=0.7)
    r = _renderer(g, tf, L, make_scene(g, 48, 40)[4], 1)
    r.set_environment(env)
    r.settings.render_mode = "raymarch"
    r.settings.bounces = 2
    r.settings.sample_range = (0.05, 1.0)
    r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
    r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
    r.render(3)                                   # frames 0..2, weight 0: the last one stays
    p = r._params
    assert p.use_env == 1 and abs(p.env_strength - 0.7) < 1e-7
    oenv = oracle.Environment(env.floats, env.width, env.height)
    want, oc = oracle.render(p, g, tf, L, frame_index=2, env=oenv)
    diff = np.abs(r.read_accum() - want).max(axis=2)
    assert (diff <= 1e-4).mean() >= 0.999, diff.max()
    r.set_environment(None)
    assert r.bind_uniforms().use_env == 0          # host falls back to the directional light
    p.use_env = 1
    r._check(r._lib.vx_set_params(r._ctx, C.byref(p)))
    assert r._lib.vx_render_frame(r._ctx, 0, 0.0) != 0
    assert b"vx_upload_environment" in r._lib.vx_last_error(r._ctx)


def test_config1_sphere_256_live_oracle(oracle):
    """BASELINE config 1: 64^3 sphere, 256x256, default white ramp, reference perspective camera"""
    from tests.common import make_scene
    from volxel_amd import synth, default_transfer_function
    vox, sp = synth.sphere(64)
    g = oracle.BrickGrid(vox, sp)
    tf, L = default_transfer_function()
    for mode, kw in (("dvr", {}), ("dvr", dict(debug_hits=True))):
        s, cam, vol, ds, p = make_scene(g, 256, 256, mode, **kw)
        want, oc = oracle.render(p, g, tf, L)
        for layout in (0, 1, 2, 4):
            r = _renderer(g, tf, L, p, layout)
            img = _render_with_params(r, p)
            c = r.counters()
            assert np.abs(img - want).max() <= 2e-6
            assert c.samples == oc.samples and c.rays == oc.rays and c.tf_samples == oc.tf_samples


def test_config1_sphere_256_ortho_live_oracle(oracle):
    """BASELINE config 1 as written: 64^3 sphere, 256x256 ORTHO ([build] parallel rays, half height 0.6; the
    reference camera is perspective only, scene.ts:65-72), default white ramp; DVR, jittered DVR and debugHits"""
    from tests.common import make_scene
    from volxel_amd import synth, default_transfer_function
    vox, sp = synth.sphere(64)
    g = oracle.BrickGrid(vox, sp)
    tf, L = default_transfer_function()
    for kw, frame in ((dict(), 0), (dict(debug_hits=True), 0), (dict(dvr_jitter=True), 3)):
        s, cam, vol, ds, p = make_scene(g, 256, 256, "dvr", ortho=0.6, **kw)
        assert p.camera_ortho == 1
        want, oc = oracle.render(p, g, tf, L, frame_index=frame)
        for layout in (0, 1, 2, 4):
            r = _renderer(g, tf, L, p, layout)
            img = _render_with_params(r, p, frame=frame)
            c = r.counters()
            assert np.abs(img - want).max() <= 2e-6
            assert c.samples == oc.samples and c.rays == oc.rays and c.tf_samples == oc.tf_samples
            r.close()
    # the host class binds the same block (Camera.ortho_half_height)
    from volxel_amd import Volxel3DRenderer
    r = Volxel3DRenderer(256, 256)
    r.setup_from_grid(g)
    r.settings.render_mode = "dvr"
    r.settings.dvr_jitter = True
    r.camera.ortho_half_height = 0.6
    pb = r.bind_uniforms()
    assert pb.camera_ortho == 1 and pb.camera_proj[:] == p.camera_proj[:] and pb.camera_proj_inv[:] == p.camera_proj_inv[:]
    assert pb.camera_view_inv[:] == p.camera_view_inv[:] and pb.dvr_jitter == 1
    r.close()


def test_device_rng_known_answers(oracle):
    """rows A1/A2 on the device itself: TEA, Wang hash, the xoshiro128++ variant (s.x + s.z, quirk Q1) and the
    u24 -> f32 conversion of random.glsl:41-106 read back word for word (vx_debug_rng), against the committed
    known answers and against the oracle on further seeds"""
    import json
    from volxel_amd import Volxel3DRenderer
    kat = json.load(open(os.path.join(GOLD, "rng_kat.json")))
    r = Volxel3DRenderer(64, 64)
    L = r._lib

    def run(op, a, b, n):
        a = np.ascontiguousarray(a, dtype=np.uint32)
        b = np.ascontiguousarray(b if b is not None else a, dtype=np.uint32)
        out = np.zeros(n, dtype=np.uint32)
        r._check(L.vx_debug_rng(r._ctx, op, a.ctypes.data, b.ctypes.data, n, out.ctypes.data))
        return out
    tea = kat["tea"]
    assert run(0, [e["v0"] for e in tea], [e["v1"] for e in tea], len(tea)).tolist() == [e["out"] for e in tea]
    wang = kat["wang"]
    assert run(1, [e["x"] for e in wang], None, len(wang)).tolist() == [e["out"] for e in wang]
    for e in kat["xoshiro"]:
        assert run(2, [e["seed"]], None, len(e["out"])).tolist() == e["out"]
    # beyond the committed vectors: pixel seeds as fragment.frag:143 forms them, long streams, float bits
    rng = np.random.default_rng(12)
    v0 = (42 * rng.integers(0, 1920 * 1080, 512, dtype=np.uint64)).astype(np.uint32)
    v1 = rng.integers(0, 2000, 512, dtype=np.uint32)
    OL = oracle.lib()
    want = [OL.vxo_tea(int(a), int(b), 32) for a, b in zip(v0, v1)]
    assert run(0, v0, v1, 512).tolist() == want
    for seed in (want[0], want[17], 0xffffffff):
        raw, flt = oracle.rng_stream(seed, 300)
        assert np.array_equal(run(2, [seed], None, 300), raw)
        assert np.array_equal(run(3, [seed], None, 300), np.asarray(flt, dtype=np.float32).view(np.uint32))
    assert L.vx_debug_rng(r._ctx, 7, v0.ctypes.data, v1.ctypes.data, 4, v0.ctypes.data) != 0   # bad op
    # the free flights' -log(1 - r) (logf's sequence without its denormal / infinity handling) against logf itself, for
    # every one of the 2^24 values a draw can take
    assert int(run(4, [0], None, 65536).astype(np.uint64).sum()) == 0
    r.close()


def test_ct_phantom_clip_anisotropic_live_oracle(oracle):
    """config 2 flavour at reduced size: anisotropic spacing, benchmark.json TF / camera /
    histogram range / multiplier, clip box, native brick builder on the product side"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import synth, read_u16_stack_to_grid
    vox, sp = synth.ct_phantom(96)
    msg = read_u16_stack_to_grid(vox, sp)        # product's preprocessor
    og = oracle.BrickGrid(vox, sp)               # oracle's
    assert np.array_equal(msg.atlas, og.atlas)
    tf, L = benchmark_tf()
    s, cam, vol, ds, p = make_scene(og, 320, 180, "dvr", sample_range=(0.05645751953125, 1.0),
                                    density_multiplier=0.99, clip_min=(0.25, 0, 0), clip_max=(1, 1, 0.75),
                                    **BENCH_CAM)
    want, oc = oracle.render(p, og, tf, L)
    for layout in (1, 2):
        r = _renderer(msg, tf, L, p, layout)
        img = _render_with_params(r, p)
        c = r.counters()
        assert np.abs(img - want).max() <= 2e-6
        assert c.samples == oc.samples


def test_progressive_accumulation_matches_oracle(oracle):
    """frames 0..7 with the viewer's sample weights (viewer.ts:1356) and per-frame jitter"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import synth, sample_weight
    vox, sp = synth.value_noise(32, seed=5, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    s, cam, vol, ds, p = make_scene(g, 64, 48, "dvr", dvr_jitter=True, sample_range=(0.05, 1.0), **BENCH_CAM)
    r = _renderer(g, tf, L, p, 2)
    prev = None
    for f in range(8):
        w = sample_weight(f)
        want, _ = oracle.render(p, g, tf, L, frame_index=f, sample_weight=w, prev=prev)
        img = _render_with_params(r, p, f, w)
        assert np.abs(img - want).max() <= 4e-6, f
        prev = want
    # the host-level render() loop does the same thing
    r2 = _renderer(g, tf, L, p, 1)
    r2.set_environment(None)           # p was built without a map: directional light
    r2.settings = s
    r2.camera = cam
    r2.render(frames=8)
    assert np.abs(r2.read_accum() - prev).max() <= 4e-6


@pytest.mark.parametrize("mode", ["default", "dvr"])
def test_derived_tables_follow_their_inputs(oracle, mode):
    """The library keeps tables derived from the transfer function and a few uniforms -- the local majorants of the
    `default` mode's DDA (dda.glsl:36,78) and the macro-cell mask of the exact empty-space skipping -- and rebuilds
    them when an input changes: after every change of TF, sample range, density multiplier or volume on ONE context
    the frame equals that of a fresh context, bit for bit, sample counts included."""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer, default_transfer_function
    grids = [oracle.BrickGrid(*small_noise(64, seed=9)), oracle.BrickGrid(*small_noise(48, seed=4))]
    tfs = [benchmark_tf(), default_transfer_function()]
    steps = [dict(g=0, tf=0, sample_range=(0.05, 1.0), density_multiplier=1.0),
             dict(g=0, tf=1, sample_range=(0.05, 1.0), density_multiplier=1.0),      # another transfer function
             dict(g=0, tf=1, sample_range=(0.3, 1.0), density_multiplier=1.0),       # another sample range
             dict(g=0, tf=1, sample_range=(0.3, 1.0), density_multiplier=0.6),       # another density scale / majorant
             dict(g=1, tf=1, sample_range=(0.3, 1.0), density_multiplier=0.6),       # another volume
             dict(g=1, tf=0, sample_range=(0.05, 1.0), density_multiplier=1.0)]      # everything back at once

    def frame(r, st, fresh):
        if fresh or r.volume is None or st["g"] != frame.g:
            r.setup_from_grid(grids[st["g"]])
        frame.g = st["g"]
        r.change_transfer_func(*tfs[st["tf"]])
        r.settings.render_mode, r.settings.bounces = mode, 2
        r.settings.dvr_skip_empty = True
        r.settings.sample_range = st["sample_range"]
        r.settings.density_multiplier = st["density_multiplier"]
        r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
        r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
        r.restart_rendering(); r.reset_counters()
        r.render(frames=2)
        c = r.counters()
        return r.read_accum(), c.samples, c.skip_steps

    frame.g = None
    kept = Volxel3DRenderer(96, 64)
    for i, st in enumerate(steps):
        a = frame(kept, st, False)
        fresh = Volxel3DRenderer(96, 64)
        b = frame(fresh, st, True)
        fresh.close()
        assert np.array_equal(a[0], b[0]) and a[1:] == b[1:] and a[1] > 0, (mode, i)
    kept.close()


@pytest.mark.parametrize("layout", [0, 1, 2, 4])
def test_empty_space_skipping_is_exact(oracle, layout):
    """skipping on/off: identical pixels, sample counts equal to the oracle's in both settings"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import synth
    inner, sp = synth.value_noise(64, seed=5, zero_quantile=0.6)
    vox = np.zeros((128, 128, 128), dtype=np.uint16)
    vox[20:84, 30:94, 40:104] = inner
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    s, cam, vol, ds, p = make_scene(g, 160, 96, "dvr", sample_range=(0.05645751953125, 1.0), **BENCH_CAM)
    r = _renderer(g, tf, L, p, layout)
    imgs, counts = [], []
    for skip in (1, 0):
        p.dvr_skip_empty = skip
        want, oc = oracle.render(p, g, tf, L)
        r.reset_counters()
        img = _render_with_params(r, p)
        c = r.counters()
        assert np.abs(img - want).max() <= 2e-6
        assert c.samples == oc.samples
        imgs.append(img); counts.append(c.samples)
    assert np.array_equal(imgs[0], imgs[1])
    assert counts[0] < counts[1]


@pytest.mark.parametrize("mode", ["dvr", "dvr_phong", "raymarch", "default", "no_dda"])
def test_pipelined_frames_are_bit_identical(oracle, mode):
    """vx_render_frames with several frames in flight == the same frames one by one"""
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    from volxel_amd import synth
    vox, sp = synth.value_noise(32, seed=5, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    s, cam, vol, ds, p = make_scene(g, 200, 120, mode, dvr_jitter=True, sample_range=(0.05, 1.0), **BENCH_CAM)
    out = []
    for in_flight in (1, 4, 8, 32, 64):
        r = _renderer(g, tf, L, p, 1)
        r.settings = s; r.camera = cam
        r.reset_counters()
        r.render(frames=3)                       # a few serial frames first
        r.render(frames=69, in_flight=in_flight)  # 64 in flight: one full launch + a partial one
        out.append((r.read_accum(), r.counters().samples, r.frame_index))
    assert out[0][2] == 72
    for img, n, fi in out[1:]:
        assert np.array_equal(img, out[0][0]) and n == out[0][1] and fi == 72


def test_display_pass_matches_blit(oracle):
    from tests.golden.make_golden import build_case
    grid, tf, L, p, frame = build_case(oracle, "noise32_dvr_clip")
    r = _renderer(grid, tf, L, p, 1)
    img = _render_with_params(r, p, frame)
    disp = r.read_display()
    want8, _ = oracle.blit(img, 5.5, 2.2)
    assert np.abs(disp.astype(int) - want8.astype(int)).max() <= 1


def test_low_resolution_preview_ramp(oracle):
    """viewer.ts:925-949,1167-1188: 0.33 x canvas for the first 5 frames after a restart, NEAREST
    blit to the canvas, then full size and the running mean starts over (viewer.ts:1356)"""
    from tests.common import benchmark_tf, BENCH_CAM
    from volxel_amd import Volxel3DRenderer, compute_params, sample_weight, synth
    vox, sp = synth.value_noise(32, seed=5, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    r = Volxel3DRenderer(96, 64, low_res_preview=True)
    r.setup_from_grid(g)
    r.change_transfer_func(tf, L)
    r.settings.render_mode = "dvr"
    r.settings.dvr_jitter = True
    r.settings.resolution_factor = 0.8
    r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
    r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
    r.restart_rendering()
    lw, lh = math.floor(96 * (0.33 * 0.8)), math.floor(64 * (0.33 * 0.8))
    assert (r.width, r.height) == (lw, lh) == (25, 16)
    r.render(3)
    assert r.frame_index == 3 and (r.width, r.height) == (lw, lh)
    env = oracle.Environment(r.environment.floats, r.environment.width, r.environment.height)
    p = compute_params(r.settings, r.camera, r.volume, r.density_scale, lw, lh, has_environment=True)
    assert p.use_env == 1                          # the viewer's default: checkerboard map, useEnv
    want, _ = oracle.render(p, g, tf, L, frame_index=2, sample_weight=0.0, env=env)
    low = r.read_accum()
    assert low.shape == (lh, lw, 4) and np.abs(low - want).max() <= 1e-5
    disp = r.read_display()
    assert disp.shape == (64, 96, 4)
    want8, _ = oracle.blit(low, r.settings.exposure, r.settings.gamma)
    ys = ((2 * np.arange(64) + 1) * lh) // (2 * 64)
    xs = ((2 * np.arange(96) + 1) * lw) // (2 * 96)
    assert np.abs(disp.astype(int) - want8[ys][:, xs].astype(int)).max() <= 1
    r.render(4, in_flight=4)                       # frames 3,4 low; 5,6 at full size
    fw, fh = math.floor(96 * 0.8), math.floor(64 * 0.8)
    assert r.frame_index == 7 and (r.width, r.height) == (fw, fh) and r.resolution_factor == 1.0
    p = compute_params(r.settings, r.camera, r.volume, r.density_scale, fw, fh, has_environment=True)
    prev = None
    for f in (5, 6):
        prev, _ = oracle.render(p, g, tf, L, frame_index=f, sample_weight=sample_weight(f), prev=prev, env=env)
    assert np.abs(r.read_accum() - prev).max() <= 1e-5
    r.restart_rendering()                          # any restart drops back to the preview size
    assert (r.width, r.height, r.frame_index) == (lw, lh, 0)
    r.render(1)
    want, _ = oracle.render(compute_params(r.settings, r.camera, r.volume, r.density_scale, lw, lh,
                                           has_environment=True), g, tf, L, frame_index=0, sample_weight=0.0, env=env)
    assert np.abs(r.read_accum() - want).max() <= 1e-5


def test_benchmark_runner_records(oracle):
    """start_benchmark (viewer.ts:856-890) + the result record of viewer.ts:1229-1241"""
    import copy
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, compute_params, sample_weight, synth
    vox, sp = synth.value_noise(32, seed=5, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    shared = copy.deepcopy(BENCHMARK_SETTINGS)
    shared["display"]["samples"] = 7
    coll = {"sharedSettings": [shared],
            "benchmarks": [{"renderMode": "raymarch", "settings": 0, "name": "rm"},
                           {"renderMode": "dvr", "settings": 0, "name": "dvr", "zip": "noise"}]}
    r = Volxel3DRenderer(96, 64)
    r.setup_from_grid(g)
    res = r.start_benchmark(coll, volumes={"noise": g})
    assert [x["name"] for x in res] == ["rm", "dvr"]
    for x in res:
        assert x["totalTime"] > 0 and abs(x["timePerSample"] - x["totalTime"] / 8) < 1e-9   # frames 0..7
        assert x["viewport"] == [0, 0, 0.8 * 96, 0.8 * 64] and x["settings"]["maxSamples"] == 7
        assert "gfx950" in x["device"]["gpu"]["renderer"] and x["timestamp"].endswith("Z")
    assert res[0]["settings"]["renderMode"] == "raymarch" and res[1]["settings"]["renderMode"] == "dvr"
    # state after the run: frames 5..7 accumulated at 0.8 x canvas, then back to the caller's sizing
    assert r.frame_index == 8
    fw, fh = math.floor(96 * 0.8), math.floor(64 * 0.8)
    with pytest.raises(Exception):
        r.start_benchmark({"sharedSettings": [shared], "benchmarks": [{"settings": 0, "zip": "missing"}]})
    # same scenario by hand == what the runner left in the accumulator
    r2 = Volxel3DRenderer(96, 64, low_res_preview=True)
    r2.setup_from_grid(g)
    r2.restore_settings(shared)
    r2.render_mode = "dvr"
    r2.render(8)
    p = compute_params(r2.settings, r2.camera, r2.volume, r2.density_scale, fw, fh, has_environment=True)
    env = oracle.Environment(r2.environment.floats, r2.environment.width, r2.environment.height)
    from tests.common import benchmark_tf
    tf, L = benchmark_tf()
    prev = None
    for f in (5, 6, 7):
        prev, _ = oracle.render(p, g, tf, L, frame_index=f, sample_weight=sample_weight(f), prev=prev, env=env)
    assert (r2.width, r2.height) == (fw, fh)
    assert np.abs(r2.read_accum() - prev).max() <= 1e-5


def test_restart_from_files_end_to_end(oracle, tmp_path):
    """row N1 through the host: DICOM slices on disk -> native reader -> brick grid -> render, equal to
    the decoded-stack path and to the oracle (restartFromFiles, viewer.ts:963-975)"""
    from tests.dicom_writer import write_slice
    from volxel_amd import Volxel3DRenderer, read_u16_stack_to_grid, synth
    vox, _ = synth.value_noise(32, seed=9, zero_quantile=0.4)
    paths = []
    for z in range(vox.shape[0]):
        paths.append(str(tmp_path / ("s%03d.dcm" % z)))
        with open(paths[-1], "wb") as f:
            f.write(write_slice(vox[z], spacing=(0.8, 0.8), thickness=1.6))
    imgs = []
    for how in ("files", "stack"):
        r = Volxel3DRenderer(80, 64)
        if how == "files":
            r.restart_from_files(paths)
        else:
            r.setup_from_grid(read_u16_stack_to_grid(vox, spacing=(0.8, 0.8, 1.6)))
        r.settings.render_mode = "dvr"
        r.render(1)
        imgs.append(r.read_accum())
    assert np.array_equal(imgs[0], imgs[1])
    from tests.common import default_environment
    g = oracle.BrickGrid(vox, (0.8, 0.8, 1.6))
    tf, L = r._tf
    want, oc = oracle.render(r._params, g, tf, L, env=default_environment(oracle))
    assert np.abs(imgs[0] - want).max() <= 1e-5 and r.counters().samples == oc.samples
    r.setup_env({"width": 4, "height": 2, "floats": np.full(4 * 2 * 4, 0.5, dtype=np.float32)})
    assert r.environment.width == 4 and r.frame_index == 0
    r.settings.debug_hits = True
    r.camera.pos = np.asarray([0.0, 0.0, -3.0])
    r.render(1)
    bg = r.read_accum()[0, 0]
    assert np.allclose(bg[:3], 0.5, atol=1e-6)           # constant map: every background pixel is 0.5


EDGE_CASES = {
    # name: (image size, make_scene kwargs, transfer-function length or None for the benchmark stops)
    "one_pixel": ((1, 1), dict(), None),
    "ragged_7x5": ((7, 5), dict(), None),
    "ragged_65x63": ((65, 63), dict(), None),                         # one pixel past the 64x64 shard tile
    "ragged_130x9": ((130, 9), dict(), None),
    "camera_inside": ((48, 40), dict(cam_pos=(0.05, 0.02, -0.1), look_at=(0.0, 0.0, 0.3)), None),
    "empty_clip_box": ((40, 32), dict(clip_min=(0.5, 0.5, 0.5), clip_max=(0.5, 0.5, 0.5)), None),
    "thin_clip_slab": ((40, 32), dict(clip_min=(0.0, 0.0, 0.49), clip_max=(1.0, 1.0, 0.51)), None),
    "range_excludes_all": ((40, 32), dict(sample_range=(2.0, 3.0)), None),
    "max_steps_10": ((40, 32), dict(dvr_max_steps=10), None),
    "step_3_voxels": ((40, 32), dict(dvr_step_voxels=3.0), None),
    "step_tiny": ((24, 16), dict(dvr_step_voxels=0.03125), None),
    "ert_off": ((40, 32), dict(dvr_ert_epsilon=1e-30), None),
    "ert_immediate": ((40, 32), dict(dvr_ert_epsilon=0.9999), None),
    "ert_epsilon_one": ((40, 32), dict(dvr_ert_epsilon=1.0), None),    # threshold tau 0: every ray ends at its first
    "ert_epsilon_two": ((40, 32), dict(dvr_ert_epsilon=2.0), None),    # contributing sample (served by render_generic)
    "dense": ((40, 32), dict(density_multiplier=50.0), None),
    "tf_len_1": ((40, 32), dict(), 1),
    "tf_len_2": ((40, 32), dict(), 2),
    "tf_len_4096": ((40, 32), dict(), 4096),                          # past the LDS-resident LUT size
}


def _edge_case_scene(oracle, case, mode):
    from tests.common import make_scene, benchmark_tf, BENCH_CAM
    (w, h), kw, tf_len = EDGE_CASES[case]
    rng = np.random.default_rng(17)
    vox = rng.integers(0, 4000, size=(11, 24, 40), dtype=np.uint16)
    vox[:, :6, :] = 0
    g = oracle.BrickGrid(vox, (0.5, 0.75, 1.25))
    if tf_len is None:
        tf, L = benchmark_tf()
    else:
        t = np.linspace(0.0, 1.0, tf_len, dtype=np.float32)
        tf = np.stack([t, 1 - t, 0.5 + 0 * t, 0.2 + 0.8 * t], axis=1).astype(np.float32).ravel()
        L = tf_len
    kw = dict(kw)
    for k, v in BENCH_CAM.items():
        kw.setdefault(k, v)
    kw.setdefault("sample_range", (0.05, 1.0))
    s, cam, vol, ds, p = make_scene(g, w, h, mode, **kw)
    return g, tf, L, kw, p


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edge_cases_match_oracle(oracle, case):
    """ragged image sizes, degenerate clip boxes / ranges / step sizes / LUT lengths, camera inside the
    volume, on a ragged (40x24x11 -> 64^3 padded) anisotropic volume: DVR == oracle with equal sample
    counts for all three layouts, one stochastic mode agrees"""
    from tests.common import make_scene
    (w, h), _, _ = EDGE_CASES[case]
    g, tf, L, kw, p = _edge_case_scene(oracle, case, "dvr")
    want, oc = oracle.render(p, g, tf, L)
    for layout in (0, 1, 2, 4):
        r = _renderer(g, tf, L, p, layout)
        r.reset_counters()
        img = _render_with_params(r, p)
        c = r.counters()
        assert img.shape == (h, w, 4)
        assert np.abs(img - want).max() <= 2e-6, (case, layout)
        assert (c.samples, c.rays, c.pixels, c.tf_samples) == (oc.samples, oc.rays, w * h, oc.tf_samples), (case, layout)
    s, cam, vol, ds, p = make_scene(g, w, h, "no_dda", **{k: v for k, v in kw.items() if not k.startswith("dvr_")})
    want, oc = oracle.render(p, g, tf, L, frame_index=1)
    r = _renderer(g, tf, L, p, 1)
    img = _render_with_params(r, p, 1)
    diff = np.abs(img - want).max(axis=2)
    assert (diff <= 1e-4).mean() >= 0.999, (case, diff.max())
    assert r.counters().rays == oc.rays


@pytest.mark.parametrize("case", sorted(EDGE_CASES))
def test_edge_cases_phong_match_oracle(oracle, case):
    """the edge cases of test_edge_cases_match_oracle in dvr_phong, on every layout (the LDS-window Phong kernel stages a
    12 x 10 x 10 window and reads +-1 voxel around every shaded sample; the generic kernel serves the reference and cellquad
    layouts, a TF past the LDS-resident LUT and ERT thresholds <= 0): the goldens' Phong tolerance, 1e-5 (the Blinn terms on
    the hardware's 1-ulp rsq / log2 / exp2 against libm), and every counter exact"""
    (w, h), _, _ = EDGE_CASES[case]
    g, tf, L, kw, p = _edge_case_scene(oracle, case, "dvr_phong")
    want, oc = oracle.render(p, g, tf, L)
    for layout in (0, 1, 2, 4):
        r = _renderer(g, tf, L, p, layout)
        r.reset_counters()
        img = _render_with_params(r, p)
        c = r.counters()
        r.close()
        assert img.shape == (h, w, 4)
        assert np.abs(img - want).max() <= 1e-5, (case, layout, float(np.abs(img - want).max()))
        assert (c.samples, c.rays, c.pixels, c.tf_samples, c.grad_samples) == \
            (oc.samples, oc.rays, w * h, oc.tf_samples, oc.grad_samples), (case, layout)


def test_upload_from_native_grid_handle(oracle):
    """vx_upload_brick_grid: builder handle -> device without the copy-out of worker.ts:19-58"""
    from volxel_amd import Volxel3DRenderer, _abi, read_u16_stack_to_grid, synth
    v1, sp = synth.value_noise(32, seed=1, zero_quantile=0.4)
    v2, _ = synth.value_noise(32, seed=2, zero_quantile=0.4)
    a = Volxel3DRenderer(64, 48)
    a.setup_from_grid(read_u16_stack_to_grid(v1, sp))
    a.settings.render_mode = "dvr"
    a.render(1)
    b = Volxel3DRenderer(64, 48)
    b.setup_from_grid(read_u16_stack_to_grid(v2, sp))       # same extent and transform, other voxels
    b.settings.render_mode = "dvr"
    b.render(1)
    assert not np.array_equal(a.read_accum(), b.read_accum())
    lib = _abi.load_library()
    vox = np.ascontiguousarray(v1, dtype=np.uint16)
    g = C.c_void_p()
    assert lib.vxb_build_from_u16(vox.ctypes.data, (C.c_uint32 * 3)(32, 32, 32), (C.c_float * 3)(*sp), 0, 2,
                                  C.byref(g)) == 0
    try:
        b._check(lib.vx_upload_brick_grid(b._ctx, g))
    finally:
        lib.vxb_free(g)
    b.restart_rendering()
    b.render(1)
    assert np.array_equal(a.read_accum(), b.read_accum())
    assert lib.vx_upload_brick_grid(b._ctx, None) != 0 and b"null grid" in lib.vx_last_error(b._ctx)


def test_error_contract():
    from volxel_amd import Volxel3DRenderer, VolxelError
    r = Volxel3DRenderer(64, 64)
    with pytest.raises(VolxelError, match="without a volume"):
        r.render()
    rc = r._lib.vx_render_frame(r._ctx, 0, 0.0)
    assert rc == 3 and b"no volume" in r._lib.vx_last_error(r._ctx)
    with pytest.raises(VolxelError, match="Unrecognized render mode"):
        r.render_mode = "fancy"
    with pytest.raises(VolxelError):
        r.resize(0, 10)
    with pytest.raises(VolxelError):
        r.change_transfer_func(np.zeros(7, dtype=np.float32), 2)
    # the DVR kernels count steps in fp32: a step limit past 2^24 could never be reached (and a zero step never ends)
    from volxel_amd import read_u16_stack_to_grid, synth
    r.setup_from_grid(read_u16_stack_to_grid(*synth.sphere(32)))
    r.settings.render_mode = "dvr"
    for field, bad in (("dvr_max_steps", (1 << 24) + 1), ("dvr_max_steps", -1), ("dvr_step_voxels", 0.0),
                       ("dvr_step_voxels", float("nan"))):
        good = getattr(r.settings, field)
        setattr(r.settings, field, bad)
        with pytest.raises(VolxelError, match=field):
            r.bind_uniforms()
        setattr(r.settings, field, good)
    p = r.bind_uniforms()
    # a clip box that reaches beyond the volume's own box (the viewer never produces one, volume.ts:32-37) is refused
    # at render time on every layout alike, instead of sampling clamped edge cells on one layout and zeros on the others
    import copy
    q = copy.copy(p)
    q.volume_aabb_max[0] = p.volume_aabb_max[0] + 0.25
    for layout in (0, 1, 2):
        r.set_layout(layout)
        r._check(r._lib.vx_set_params(r._ctx, C.byref(q)))
        assert r._lib.vx_render_frame(r._ctx, 0, 0.0) == 1 and b"outside the volume" in r._lib.vx_last_error(r._ctx)
    r._check(r._lib.vx_set_params(r._ctx, C.byref(p)))
    r._check(r._lib.vx_render_frame(r._ctx, 0, 0.0))


def test_host_rejects_arrays_shorter_than_their_size_fields(oracle):
    """the C ABI takes raw pointers: the binding checks lengths before the call"""
    import copy
    from volxel_amd import Volxel3DRenderer, VolxelError, synth
    vox, sp = synth.sphere(32)
    g = oracle.BrickGrid(vox, sp)
    r = Volxel3DRenderer(64, 64)
    for field in ("indirection", "range", "atlas"):
        bad = copy.copy(g)
        setattr(bad, field, np.asarray(getattr(g, field))[:-8])
        with pytest.raises(VolxelError, match=field):
            r.setup_from_grid(bad)
    bad = copy.copy(g)
    bad.range_mipmaps = [(np.asarray(m)[:-2], st) for m, st in g.range_mipmaps]
    with pytest.raises(VolxelError, match="mipmap"):
        r.setup_from_grid(bad)
    r.setup_from_grid(g)          # the intact grid still loads
    r.close()


def test_counters_report_the_launches_that_ran(oracle):
    """vx_get_counters: frames per launch as launched (not as requested), gather instructions of the tuned
    kernel, the blend time apart from the render time"""
    from tests.common import benchmark_tf
    from volxel_amd import Volxel3DRenderer, synth
    vox, sp = synth.value_noise(64, seed=2, zero_quantile=0.4)
    g = oracle.BrickGrid(vox, sp)
    r = Volxel3DRenderer(192, 128, layout=1)                  # the cellquad gather kernel and its probes
    r.setup_from_grid(g)
    r.change_transfer_func(*benchmark_tf())
    r.settings.render_mode = "dvr"
    r.settings.dvr_jitter = True
    r.settings.dvr_skip_empty = False
    r.render(frames=2); r.finish(); r.reset_counters()       # the first frames build the launch order one by one
    r.render(frames=20, rebind=False, in_flight=64); r.finish()
    c = r.counters()
    assert (c.launches, c.frames, c.min_launch_frames, c.max_launch_frames) == (1, 20, 20, 20)
    assert c.merge_ms > 0 and c.kernel_ms > 0 and c.merge_launches == 1
    # 2 gathers per march step, issued in batches of 4 steps: between 2 per wave step and that plus one batch per wave
    steps = c.lane_slots // 64
    waves = 20 * (192 // 8) * (128 // 8)
    assert 2 * steps <= c.gathers <= 2 * steps + 8 * waves + 8 * 20 * 4 * 16
    r.reset_counters()
    r.render(frames=7, rebind=False, in_flight=3); r.finish()
    c = r.counters()
    assert (c.launches, c.frames, c.min_launch_frames, c.max_launch_frames) == (3, 7, 1, 3)
    # the spread probe marches the same rays: same gather count per frame, at least one line per quad of lanes
    r.restart_rendering(); r.reset_counters(); r.render(); r.finish()
    one = r.counters()
    n, lines, quads = r.probe_gather_spread(0)
    assert 2 * n == one.gathers
    assert n <= lines <= 64 * n and lines <= quads <= 64 * n and 16 * n >= quads // 4
    clk, khz = r.probe_gather_rate(16)
    clk1, _ = r.probe_gather_rate(1)
    clk64, _ = r.probe_gather_rate(64)
    clk30_10, _ = r.probe_gather_rate(30, 10)     # 30 line look-ups over 10 distinct lines, the shape of the march
    clk30, _ = r.probe_gather_rate(30)
    assert khz >= 1000000 and 10.0 < clk1 <= clk < clk64 < 400.0 and clk <= clk30_10 <= clk30 * 1.05
    r.close()
    # the default layout (VX_LAYOUT_AUTO) marches DVR through LDS windows: staging loads and LDS tap reads are counted
    r = Volxel3DRenderer(192, 128)
    r.setup_from_grid(g)
    r.change_transfer_func(*benchmark_tf())
    r.settings.render_mode = "dvr"
    r.settings.dvr_skip_empty = False
    r.render(frames=2); r.finish(); r.reset_counters()
    r.render(frames=5, rebind=False, in_flight=5); r.finish()
    c = r.counters()
    steps = c.lane_slots // 64
    assert (c.launches, c.max_launch_frames) == (1, 5) and c.lds_reads == 4 * steps and 0 < c.gathers < steps
    with pytest.raises(Exception, match="cellquad"):
        r.probe_gather_spread(0)
    r.close()


# ---- full-size (BASELINE config 3: 512^3, 1080p) through size-independent properties --------
@pytest.fixture(scope="module")
def big_scene():
    from volxel_amd import synth, read_u16_stack_to_grid, Volxel3DRenderer, BENCHMARK_SETTINGS
    vox, sp = synth.value_noise(512, seed=42)
    msg = read_u16_stack_to_grid(vox, sp)
    del vox
    r = Volxel3DRenderer(1920, 1080)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.render_mode = "dvr"
    r.settings.volume_clip_min = (0.25, 0.0, 0.0)
    r.settings.volume_clip_max = (1.0, 1.0, 0.75)
    return r, msg


def test_fullsize_properties(big_scene):
    r, msg = big_scene
    r.restart_rendering(); r.reset_counters()
    r.render()
    base = r.read_accum()
    c0 = r.counters()
    assert np.isfinite(base).all() and base[..., 3].min() == 1.0
    assert c0.pixels == 1920 * 1080 and c0.samples > 1e8
    # (a) idempotence / determinism: same frame index -> identical bits
    r.restart_rendering(); r.render()
    assert np.array_equal(r.read_accum(), base)
    # (b) layout independence: every layout / kernel gives the same densities, bins, counts
    for layout in (0, 1):
        r.set_layout(layout); r.restart_rendering(); r.reset_counters(); r.render()
        ref_img = r.read_accum(); c1 = r.counters()
        assert c1.samples == c0.samples and c1.rays == c0.rays
        assert np.abs(ref_img - base).max() <= 2e-6
    r.set_layout(2)
    # (c) linearity in the light: doubling env_strength doubles every pixel exactly
    r.env_strength = 2.0; r.restart_rendering(); r.render()
    assert np.array_equal(r.read_accum()[..., :3], base[..., :3] * 2)
    r.env_strength = 1.0
    # (d) early ray termination only removes what lies below the threshold
    eps = r.settings.dvr_ert_epsilon
    r.settings.dvr_ert_epsilon = 1e-9; r.restart_rendering(); r.reset_counters(); r.render()
    full = r.read_accum(); c2 = r.counters()
    r.settings.dvr_ert_epsilon = eps
    assert c2.samples >= c0.samples
    assert np.abs(full - base).max() <= eps * 4.02 + 1e-6
    # (e) a clip box at the volume's own bounds equals no clipping of a sub-box union:
    #     rendering with clip_min.x = 0.25 must see no sample left of that plane
    #     -> equal to rendering the mirrored camera... (covered by oracle parity at small size)


@pytest.mark.parametrize("mode", ["dvr", "dvr_phong"])
def test_fullsize_config3_config4_match_live_oracle(big_scene, oracle, mode):
    """BASELINE configs 3 and 4 at their full size -- 512^3, 1920x1080, clip box, ERT, per-frame jitter on; config 4
    adds the central-difference gradient and Blinn-Phong -- against the CPU oracle on the same frame (16 host threads
    render the 214 M samples of the frame in about a second): every pixel within the fp tolerance, exact sample,
    ray and shaded-sample counts.  Frame 5 through a 3-frame launch, i.e. the multi-frame path and the blend."""
    r, msg = big_scene
    r.set_layout(3)
    old = (r.settings.render_mode, r.settings.dvr_jitter, r.settings.dvr_skip_empty)
    # config 3 marches every sample (the bench's setting); config 4 here with exact empty-space skipping on
    r.settings.render_mode, r.settings.dvr_jitter, r.settings.dvr_skip_empty = mode, True, mode == "dvr_phong"
    try:
        p = r.bind_uniforms()
        r.restart_rendering(); r.reset_counters()
        r._check(r._lib.vx_render_frame(r._ctx, 5, 0.0))
        img = r.read_accum(); c = r.counters()
        vol = oracle.make_volume(msg)
        want, oc = oracle.render(p, vol, *r._tf, frame_index=5, threads=16, env=_oracle_env(oracle, r))
        # the composite's exp is the hardware's 1-ulp v_exp_f32, the oracle's libm's: over rays of up to 1500 samples
        # the colour sums drift apart by a few 1e-6 (small cases: 2e-6) -- a tenth of BASELINE.md's 1e-4 budget
        tol = 2e-5 if mode == "dvr_phong" else 1e-5
        assert float(np.abs(img - want).max()) <= tol
        assert (c.samples, c.rays, c.pixels, c.tf_samples) == (oc.samples, oc.rays, 1920 * 1080, oc.tf_samples)
        assert c.samples > (1.4e8 if r.settings.dvr_skip_empty else 2.1e8)
        if mode == "dvr_phong":
            assert c.grad_samples == oc.grad_samples and c.grad_samples > 1e7
        # the same frame as the last of a 3-frame launch (weights 0: the accumulator keeps the last frame)
        r.restart_rendering()
        w = (C.c_float * 3)(0.0, 0.0, 0.0)
        r._check(r._lib.vx_render_frames(r._ctx, 3, 3, w, 3))
        assert np.array_equal(r.read_accum(), img)
    finally:
        r.settings.render_mode, r.settings.dvr_jitter, r.settings.dvr_skip_empty = old


def _check_reference_mode_frame(r, msg, oracle, mode, frame, rect=None, launch_frames=8):
    """one accumulation frame of a reference render mode (dda.glsl:65-98 `default`, normal.glsl:33-57 `no_dda`,
    raymarch.glsl:25-55 `raymarch`, each under fragment.frag:79-124) at the scene's full size against the live oracle:
    through vx_render_frame (one pixel per lane) and as the LAST frame of a `launch_frames`-frame vx_render_frames launch
    (lanes = pixels x frames).  The small goldens' criteria: >= 99.9 % of the pixels within 1e-4 (a 1-ulp
    log() can flip one collision decision and re-roll that pixel), samples and DDA steps within 0.2 %, rays counted
    exactly as the oracle's when no decision flipped (within 0.2 % otherwise)."""
    W, H = r.width, r.height
    old = (r.settings.render_mode, r.settings.bounces)
    r.settings.render_mode = mode
    try:
        p = r.bind_uniforms()
        r.restart_rendering(); r.reset_counters()
        r._check(r._lib.vx_render_frame(r._ctx, frame, 0.0))
        img = r.read_accum(); c = r.counters()
        assert c.pixels == W * H and np.isfinite(img).all()
        # the same frame as the last of a multi-frame launch (weights 0: the accumulator keeps the last frame)
        r.restart_rendering(); r.reset_counters()
        w = (C.c_float * launch_frames)(*([0.0] * launch_frames))
        r._check(r._lib.vx_render_frames(r._ctx, frame - launch_frames + 1, launch_frames, w, launch_frames))
        img_n = r.read_accum(); cn = r.counters()
        assert cn.max_launch_frames == launch_frames and cn.launches == 1
        assert np.array_equal(img_n, img), mode            # HIP against HIP: bit for bit
        x0, x1, y0, y1 = rect if rect else (0, W, 0, H)
        want, oc = oracle.render(p, oracle.make_volume(msg), *r._tf, frame_index=frame, rect=(x0, x1, y0, y1),
                                 threads=16, env=_oracle_env(oracle, r))
        diff = np.abs(img[y0:y1, x0:x1] - want[y0:y1, x0:x1]).max(axis=2)
        frac = float((diff <= 1e-4).mean())
        print(f"full size {mode}: {frac * 100:.4f} % of {diff.size} pixels within 1e-4, {int((diff > 1e-4).sum())} re-rolled, "
              f"oracle samples {oc.samples} rays {oc.rays} steps {oc.skip_steps}")
        assert frac >= 0.999, (mode, frac, float(diff.max()))
        if rect is None:
            assert abs(int(c.samples) - int(oc.samples)) <= 0.002 * oc.samples + 64, (c.samples, oc.samples)
            assert abs(int(c.skip_steps) - int(oc.skip_steps)) <= 0.002 * oc.skip_steps + 64, (c.skip_steps, oc.skip_steps)
            assert abs(int(c.rays) - int(oc.rays)) <= 0.002 * oc.rays + 64, (c.rays, oc.rays)
            if mode == "default":
                assert oc.skip_steps > oc.samples > 1e6       # the DDA really walks at this size
            else:
                assert oc.samples > 1e7
        return frac
    finally:
        r.settings.render_mode, r.settings.bounces = old
        r.bind_uniforms()


@pytest.mark.parametrize("mode", ["default", "no_dda", "raymarch"])
def test_fullsize_reference_modes_match_live_oracle(big_scene, oracle, mode):
    """the reference's own three render modes on the BASELINE config-3 scene -- 512^3, 1920x1080, clip box, the benchmark's
    transfer function and camera -- on the AUTO layout (the 2.5 GB cellquad build and its 24-bit brick index arithmetic for
    the trilinear modes, the majorant tables of the DDA), the whole 1080p frame against the oracle."""
    r, msg = big_scene
    r.set_layout(3)
    _check_reference_mode_frame(r, msg, oracle, mode, frame=9)


def test_fullsize_config2_ct_phantom_matches_live_oracle(oracle):
    """BASELINE config 2 at its full size: a 256^3 CT stack as 256 DICOM slices (explicit VR little endian, 12 bits
    stored) through the native DICOM reader and brick builder, 1920x1080, trilinear + 1-D transfer function, jitter on;
    exact empty-space skipping off and on (free flight over the air around the body) against the CPU oracle on the
    same frame"""
    from tests.dicom_writer import write_slice
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_dicoms_to_grid, read_u16_stack_to_grid, synth
    vox, sp = synth.ct_phantom(256)
    files = [write_slice(vox[z], spacing=(sp[0], sp[1]), thickness=sp[2]) for z in range(vox.shape[0])]
    msg = read_dicoms_to_grid(files)
    ref = read_u16_stack_to_grid(vox, sp)             # the same voxels handed over as a decoded stack
    for f in ("indirection", "range", "atlas", "index_extent", "atlas_size"):
        assert np.array_equal(np.asarray(getattr(msg, f)), np.asarray(getattr(ref, f))), f
    del files, ref
    r = Volxel3DRenderer(1920, 1080)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)       # benchmark.json: TF, histogram range, camera, multiplier
    r.settings.render_mode, r.settings.dvr_jitter = "dvr", True
    vol = oracle.make_volume(msg)
    seen = []
    for skip in (False, True):
        r.settings.dvr_skip_empty = skip
        p = r.bind_uniforms()
        r.restart_rendering(); r.reset_counters()
        r._check(r._lib.vx_render_frame(r._ctx, 2, 0.0))
        img = r.read_accum(); c = r.counters()
        want, oc = oracle.render(p, vol, *r._tf, frame_index=2, threads=16, env=_oracle_env(oracle, r))
        assert float(np.abs(img - want).max()) <= 1e-5
        assert (c.samples, c.rays, c.tf_samples) == (oc.samples, oc.rays, oc.tf_samples)
        seen.append((img, c.samples))
    assert np.array_equal(seen[0][0], seen[1][0]) and seen[1][1] < 0.5 * seen[0][1]
    r.close()


def test_fullsize_tile_shards_are_bit_identical(big_scene):
    """image-space tiles: 3 shards rendered by 3 contexts on this GPU, slabs gathered
    (device-to-device) and de-tiled == the unsharded image, bit for bit"""
    import torch
    from volxel_amd import Volxel3DRenderer
    from volxel_amd.dist import slab_tensor
    r, msg = big_scene
    r.restart_rendering(); r.render(); base = r.read_accum()
    N = 3
    slabs, total = [], 0
    for rank in range(N):
        rr = Volxel3DRenderer(1920, 1080, shard_rank=rank, shard_count=N)
        rr.setup_from_grid(msg)
        rr.settings = r.settings; rr.camera = r.camera; rr.env_strength = r.env_strength
        rr.change_transfer_func(*r._tf)
        rr.reset_counters(); rr.render(); rr.finish()
        total += rr.counters().samples
        slabs.append(slab_tensor(rr).clone())
        keep = rr
    r.reset_counters(); r.restart_rendering(); r.render()
    assert total == r.counters().samples
    gathered = torch.cat(slabs)
    image = torch.empty(1080 * 1920 * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    keep.detile(gathered.data_ptr(), image.data_ptr()); keep.finish()
    assert np.array_equal(image.view(1080, 1920, 4).cpu().numpy(), base)


def test_balanced_tile_order_is_bit_identical_and_levels_the_shards(big_scene):
    """vx_probe_tile_costs / vx_set_tile_order: every shard derives the same dealing order from the probe,
    the gathered image stays bit-identical to the unsharded one, the shard with the most samples is closer
    to the mean than with the default round-robin dealing, the tuned kernel + 32 frames per launch included"""
    import torch
    from volxel_amd import Volxel3DRenderer, tiles
    from volxel_amd.dist import slab_tensor
    r, msg = big_scene
    r.set_layout(3)                             # VX_LAYOUT_AUTO: the shard contexts below use the default layout and kernel too
    r.restart_rendering(); r.render(frames=3, in_flight=1); base = r.read_accum()
    N = 8
    perms, slabs, per_rank, plain = [], [], [], []
    for rank in (0, 3, 7):                      # three of the eight shards are enough for the image check
        rr = Volxel3DRenderer(1920, 1080, shard_rank=rank, shard_count=N)
        rr.setup_from_grid(msg)
        rr.settings = r.settings; rr.camera = r.camera; rr.env_strength = r.env_strength
        rr.change_transfer_func(*r._tf)
        rr.reset_counters(); rr.render(); rr.finish()
        c = rr.counters()
        plain.append(c.samples + c.skip_steps)
        perms.append(rr.balance_tiles())
        rr.reset_counters(); rr.render(frames=3, in_flight=1); rr.finish()
        c = rr.counters()
        per_rank.append((c.samples + c.skip_steps) // 3)
        slabs.append((rank, slab_tensor(rr).clone()))
        keep = rr
    assert all(np.array_equal(perms[0], q) for q in perms[1:])
    costs = keep.probe_tile_costs()
    assert costs.shape == (510,) and costs.max() > 0 and np.array_equal(perms[0], tiles.balanced_order(costs, N))
    gathered = torch.zeros(N * slabs[0][1].numel(), dtype=torch.float32, device="cuda")
    for rank, sl in slabs:
        gathered[rank * sl.numel():(rank + 1) * sl.numel()] = sl
    image = torch.empty(1080 * 1920 * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    keep.detile(gathered.data_ptr(), image.data_ptr()); keep.finish()
    img = image.view(1080, 1920, 4).cpu().numpy()
    px, py = [], []
    for rank, _ in slabs:                       # pixels owned by the three rendered shards
        x, y = tiles.slab_pixel_coords(1920, 1080, rank, N, perms[0])
        ok = x >= 0
        px.append(x[ok]); py.append(y[ok])
    px, py = np.concatenate(px), np.concatenate(py)
    assert np.array_equal(img[py, px], base[py, px])
    r.reset_counters(); r.restart_rendering(); r.render()
    c = r.counters()
    mean = (c.samples + c.skip_steps) / N       # the probe's cost: marched steps, evaluated or skipped
    dev = lambda xs: max(abs(x - mean) for x in xs) / mean
    assert dev(per_rank) < 0.03 and dev(per_rank) < dev(plain), (dev(per_rank), dev(plain))
    keep.set_tile_order(None)                   # back to the default dealing
    keep.reset_counters(); keep.render(); keep.finish()
    c = keep.counters()
    assert c.samples + c.skip_steps == plain[-1]
    with pytest.raises(Exception, match="permutation"):
        keep.set_tile_order(np.zeros(510, dtype=np.uint32))


# ---- BASELINE config 5: 1024^3 bricked volume, 3840x2160, 8 image-tile shards -----------------
@pytest.fixture(scope="module")
def huge_scene():
    from volxel_amd import synth, read_u16_stack_to_grid, Volxel3DRenderer, BENCHMARK_SETTINGS
    vox, sp = synth.value_noise(1024, seed=42)
    msg = read_u16_stack_to_grid(vox, sp)
    del vox
    r = Volxel3DRenderer(3840, 2160)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.render_mode = "dvr"
    r.settings.volume_clip_min = (0.25, 0.0, 0.0)
    r.settings.volume_clip_max = (1.0, 1.0, 0.75)
    r.settings.dvr_jitter = True
    yield r, msg
    r.close()


def test_config5_1024_cubed_4k_eight_tile_shards(huge_scene, oracle):
    """the brickf32 / LDS-window march, the 19.8 GB cellquad build, the 24-bit brick index arithmetic of the gather
    march, the 2040-tile dealing order and the multi-frame launch at their full size (brick.rs:77-81 sets the limits): every one of the 8 shards, dealt
    by the balanced order, reproduces its pixels of the unsharded 4K frame bit for bit; sample counts add up;
    the tuned kernel equals the generic kernel on the reference layout"""
    import torch
    from volxel_amd import Volxel3DRenderer, tiles
    from volxel_amd.dist import slab_tensor
    r, msg = huge_scene
    assert tuple(msg.indirection_size) == (128, 128, 128)
    secs, nbytes, pinned = r.upload_stats()
    assert nbytes >= msg.atlas.size and secs > 0
    r.restart_rendering(); r.reset_counters()
    r.render(frames=3, in_flight=1)              # frames 0..2, jittered: distinct rays per frame
    base = r.read_accum(); c0 = r.counters()
    assert np.isfinite(base).all() and base[..., 3].min() == 1.0
    assert c0.pixels == 3 * 3840 * 2160 and c0.samples > 2e9
    # multi-frame launch == frame by frame
    r.restart_rendering(); r.reset_counters()
    r.render(frames=3, in_flight=3)
    assert np.array_equal(r.read_accum(), base) and r.counters().samples == c0.samples
    # the default layout marches through LDS windows of the 4.3 GB brickf32 layout; the cellquad gather kernel
    # (19.8 GB build, 24-bit brick index arithmetic) and the generic kernel on the reference textures (every tap
    # through range -> pointer -> atlas) evaluate the same samples: same count, image within the exp tolerance
    for layout in (1, 0, 4):
        r.set_layout(layout); r.restart_rendering(); r.reset_counters(); r.render(frames=3, in_flight=1)
        ref = r.read_accum(); c1 = r.counters()
        assert c1.samples == c0.samples and c1.rays == c0.rays, layout
        assert np.abs(ref - base).max() <= 2e-6, layout
    r.set_layout(3)
    # against the CPU oracle: the centred 960x540 crop of frame 1 (a quarter of a billion samples)
    p = r.bind_uniforms()
    r.restart_rendering(); r.reset_counters()
    r._check(r._lib.vx_render_frame(r._ctx, 1, 0.0))
    img = r.read_accum()
    x0, y0 = (3840 - 960) // 2, (2160 - 540) // 2
    want, oc = oracle.render(p, oracle.make_volume(msg), *r._tf, frame_index=1, rect=(x0, x0 + 960, y0, y0 + 540),
                             threads=16, env=_oracle_env(oracle, r))
    assert oc.samples > 1e8
    assert float(np.abs(img[y0:y0 + 540, x0:x0 + 960] - want[y0:y0 + 540, x0:x0 + 960]).max()) <= 1e-5
    # 8 shards through ONE extra context (re-sharded in place; the volume is replicated per GPU in production)
    N = 8
    rr = Volxel3DRenderer(3840, 2160, shard_rank=0, shard_count=N)
    rr.setup_from_grid(msg)
    rr.settings = r.settings; rr.camera = r.camera; rr.env_strength = r.env_strength
    rr.change_transfer_func(*r._tf)
    perm = rr.balance_tiles()
    assert sorted(perm.tolist()) == list(range(2040))
    gathered = None
    total, per_rank = 0, []
    for rank in range(N):
        rr.shard_rank = rank
        rr.restart_rendering(); rr.reset_counters()
        rr.render(frames=3, in_flight=3); rr.finish()
        c = rr.counters()
        total += c.samples
        per_rank.append(c.samples + c.skip_steps)
        sl = slab_tensor(rr)
        if gathered is None:
            gathered = torch.zeros(N * sl.numel(), dtype=torch.float32, device="cuda")
        gathered[rank * sl.numel():(rank + 1) * sl.numel()] = sl
    assert total == c0.samples
    image = torch.empty(2160 * 3840 * 4, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    rr.detile(gathered.data_ptr(), image.data_ptr()); rr.finish()
    assert np.array_equal(image.view(2160, 3840, 4).cpu().numpy(), base)
    mean = sum(per_rank) / N
    assert max(abs(x - mean) for x in per_rank) / mean < 0.03
    rr.close()


@pytest.mark.parametrize("mode", ["default", "no_dda", "raymarch"])
def test_config5_reference_modes_crop_matches_live_oracle(huge_scene, oracle, mode):
    """the reference's modes on the 1024^3 volume at 3840x2160 (AUTO layout: 19.8 GB of cell quads, 128^3 bricks, three
    majorant mips): the centred 960x540 crop of one frame against the oracle -- the crop bounds the oracle's time, the
    device renders the whole 4K frame, alone and as the last of a 4-frame launch"""
    r, msg = huge_scene
    r.set_layout(3)
    x0, y0 = (3840 - 960) // 2, (2160 - 540) // 2
    _check_reference_mode_frame(r, msg, oracle, mode, frame=6, rect=(x0, x0 + 960, y0, y0 + 540), launch_frames=4)


def test_volume_beyond_the_cellquad_index_range_is_refused(oracle):
    """more than 2^32 quads (about 1550^3 voxels) cannot be indexed by the march's 32-bit quad offsets:
    vx_upload_volume says so and names the layouts that work (vx_api_volume.hip alloc_one_layout); brick.rs:77-81 allows
    up to 1016 bricks per axis"""
    from types import SimpleNamespace
    from volxel_amd import Volxel3DRenderer, VolxelError
    b = 200                                       # 200^3 all-constant bricks: (201^3) * 576 quads > 2^32
    n = b ** 3
    msg = SimpleNamespace(
        indirection=np.zeros(n, dtype=np.uint32), indirection_size=(b, b, b),
        range=np.zeros(2 * n, dtype=np.uint16), range_size=(b, b, b),
        atlas=np.zeros(0, dtype=np.uint8), atlas_size=(b * 8, b * 8, 0),
        range_mipmaps=[(np.zeros(2 * (b >> k) ** 3, dtype=np.uint16), (b >> k, b >> k, b >> k)) for k in (1, 2, 3)],
        index_extent=(b * 8, b * 8, b * 8), min_maj=(0.0, 1.0),
        transform=np.eye(4, dtype=np.float32).reshape(-1))
    r = Volxel3DRenderer(64, 64, layout=1)
    with pytest.raises(VolxelError, match="too large for the cellquad layout"):
        r.setup_from_grid(msg)
    with pytest.raises(VolxelError, match="without a volume|no volume"):
        r.render()
    r.set_layout(0)                               # the reference textures have no such limit
    r.setup_from_grid(msg)
    r.settings.render_mode = "dvr"
    r.render(); img = r.read_accum()
    assert np.isfinite(img).all()
    # the default (VX_LAYOUT_AUTO) takes the volume: DVR on brickf32, and the path-traced modes step down to the
    # resident fp32 bricks because cellquad cannot index it (round 4: measured 2x faster than the reference textures there)
    r.set_layout(3)
    r.render(); assert np.array_equal(r.read_accum(), img)
    r.settings.render_mode = "no_dda"
    r.render(); assert np.isfinite(r.read_accum()).all()
    r.close()


@pytest.mark.parametrize("mode", ["dvr", "dvr_phong", "default", "no_dda", "raymarch"])
def test_running_mean_in_the_render_kernel_is_bit_identical(oracle, monkeypatch, mode):
    """MultiOut::fuse (round 4): in a launch of exactly 32 or 64 frames a wave of the LDS-window kernel holds every frame of its
    2 (or 1) pixels and folds their results into the accumulator itself, in frame order, with the fma of fragment.frag:158 --
    no per-frame result slabs, no blend kernel.  Against VX_DVR_FUSE=0 (result slabs + merge_results) and against the same
    frames one by one: the same bits, with and without zero weights in the launch (the first frames of an accumulation
    carry weight 0: merge_results drops the previous value there), on a ragged image, for 32 and 64 frames in flight and a
    request that ends in a partial launch (which takes the unfused path).  The reference's three modes do the same in
    render_generic for launches of exactly 32 frames (2 pixels x 32 frames per wave, the workgroup's beam unchanged)."""
    from tests.common import benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer
    vox, sp = small_noise(64, seed=13)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    res = {}
    for key, fuse, fpl in (("serial", "1", 1), ("merge32", "0", 32), ("fused32", "1", 32), ("fused64", "1", 64), ("fused8", "1", 8),
                           ("fused16", "1", 16)):
        monkeypatch.setenv("VX_DVR_FUSE", fuse)
        r = Volxel3DRenderer(203, 131)
        r.setup_from_grid(g)
        r.change_transfer_func(tf, L)
        r.settings.render_mode, r.settings.dvr_jitter, r.settings.dvr_skip_empty = mode, True, False
        r.settings.sample_range, r.settings.bounces, r.settings.max_samples = (0.05, 1.0), 2, 1 << 20
        r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
        r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
        r.reset_counters()
        r.render(frames=2)                                  # the two frames that build the launch order
        r.render(frames=64 + 64 + 7, in_flight=fpl)         # frames 2 .. 136: launches with zero weights, without, and a partial one
        c = r.counters()
        res[key] = (r.read_accum(), c.samples, c.tf_samples, c.merge_ms, c.max_launch_frames, c.merge_launches)
        r.close()
    assert res["merge32"][3] > 0.0 and res["merge32"][4] == 32
    assert res["fused64"][4] == 64
    for key in ("merge32", "fused32", "fused64", "fused8", "fused16"):
        assert np.array_equal(res[key][0], res["serial"][0]) and res[key][1:3] == res["serial"][1:3], key
    # blend kernels launched (VxCounters.merge_launches).  The 135 frames go as 4x32+7, 2x64+7, 16x8+7 or 8x16+7 frames per
    # launch; in_flight=1 renders them frame by frame, without a blend.  DVR / Phong: both preamble frames go one by one (they
    # build the launch order) and every full launch folds, so only the 7-frame launch blends.  The reference's modes fold
    # only launches of exactly 32 frames, and the second frame of their preamble (in_flight=32 in every run) is already a
    # 1-frame multi-frame launch: one blend more in every run, `serial` included.
    if mode in ("dvr", "dvr_phong"):
        want = {"serial": 0, "merge32": 5, "fused32": 1, "fused64": 1, "fused8": 1, "fused16": 1}
    else:
        want = {"serial": 1, "merge32": 6, "fused32": 2, "fused64": 4, "fused8": 18, "fused16": 10}
    assert {key: res[key][5] for key in want} == want


@pytest.mark.parametrize("res", [(1920, 1080), (333, 251), (1000, 7), (4096, 16)])
def test_host_decided_ray_divisions_are_exact(oracle, monkeypatch, res):
    """round 4: two of a primary ray's divisions are decided per launch on the host (DevVolume::ray_flags): the three divisions by
    the w of inverse(view) * (v, 1) are skipped when that w is 1.0 by construction, and (pixel + 0.5) / res becomes a
    reciprocal product corrected by its remainder when the host found that form equal to the IEEE division for EVERY pixel
    coordinate of the resolution.  VX_RAY_SHORTCUTS=0 keeps the divisions: debugHits (the entry point of every primary ray, jitter
    included) and a jittered DVR frame must not move by a bit, whatever the resolution."""
    from tests.common import benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer
    vox, sp = small_noise(32, seed=4)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    out = {}
    for sc in ("1", "0"):
        monkeypatch.setenv("VX_RAY_SHORTCUTS", sc)
        r = Volxel3DRenderer(*res)
        r.setup_from_grid(g)
        r.change_transfer_func(tf, L)
        r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
        r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
        imgs = []
        for mode, dbg in (("dvr", True), ("dvr", False), ("no_dda", False)):
            r.settings.render_mode, r.settings.debug_hits, r.settings.dvr_jitter = mode, dbg, True
            r.restart_rendering(); r.reset_counters()
            r.render(frames=3, in_flight=3)
            imgs.append((r.read_accum(), r.counters().samples))
        out[sc] = imgs
        r.close()
    for (a, na), (b, nb) in zip(out["1"], out["0"]):
        assert np.array_equal(a, b) and na == nb


def test_auto_layout_steps_down_when_cellquad_exceeds_its_memory_budget(oracle, monkeypatch):
    """VX_LAYOUT_AUTO builds the 18-byte-per-voxel cellquad layout for `default` / `no_dda` on first use -- only inside a
    device-memory budget (half of the free memory; VX_AUTO_CELLQUAD_MAX_BYTES overrides).  Outside it the modes sample the
    resident fp32 bricks: the same densities, bins and counts (layouts are bit-identical, test_golden_stochastic_modes),
    no allocation."""
    import torch
    from tests.common import benchmark_tf, BENCH_CAM, small_noise
    from volxel_amd import Volxel3DRenderer
    vox, sp = small_noise(64, seed=9)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()
    out = {}
    for budget in (None, "0"):
        if budget is None:
            monkeypatch.delenv("VX_AUTO_CELLQUAD_MAX_BYTES", raising=False)
        else:
            monkeypatch.setenv("VX_AUTO_CELLQUAD_MAX_BYTES", budget)
        r = Volxel3DRenderer(160, 96)
        r.setup_from_grid(g)
        r.change_transfer_func(tf, L)
        r.settings.render_mode, r.settings.bounces = "no_dda", 2
        r.camera.pos = np.asarray(BENCH_CAM["cam_pos"], dtype=np.float64)
        r.camera.view = np.asarray(BENCH_CAM["look_at"], dtype=np.float64)
        torch.cuda.synchronize()
        before = torch.cuda.mem_get_info()[0]
        r.reset_counters(); r.render(frames=3, in_flight=3); r.finish()
        after = torch.cuda.mem_get_info()[0]
        c = r.counters()
        out[budget] = (r.read_accum(), c.samples, c.rays, before - after)
        r.close()
    assert np.array_equal(out[None][0], out["0"][0]) and out[None][1:3] == out["0"][1:3]
    quads = 9 ** 3 * 576 * 16                       # (8 + 1)^3 apron bricks x 576 quads x 16 bytes
    # the build happened inside the default budget and not with a budget of zero (everything else a first render
    # allocates -- result slabs, counter records -- is the same in both)
    assert out[None][3] - out["0"][3] >= quads // 2, (out[None][3], out["0"][3], quads)


def test_context_lifecycle_releases_device_memory(oracle):
    """create / upload / every kind of render / resize / layout switch / destroy, twenty times: the free
    device memory comes back (no leaked slabs, pipes, layouts, environment or order tables)"""
    import gc
    import torch
    from tests.common import benchmark_tf
    from volxel_amd import Environment, Volxel3DRenderer, synth
    vox, sp = synth.value_noise(64, seed=3, zero_quantile=0.5)
    g = oracle.BrickGrid(vox, sp)
    tf, L = benchmark_tf()

    def cycle(i):
        r = Volxel3DRenderer(320 + 8 * i, 200, shard_rank=i % 2, shard_count=2, low_res_preview=bool(i & 1))
        r.setup_from_grid(g)
        r.change_transfer_func(tf, L)
        r.set_environment(Environment(np.full((4, 8, 4), 0.5, dtype=np.float32), 8, 4))
        for mode in ("dvr", "default", "dvr_phong"):
            r.render_mode = mode
            r.render(frames=12, in_flight=8)
        r.balance_tiles()
        r.set_layout(2)
        r.settings.render_mode = "dvr"
        r.render(frames=6, in_flight=4)
        r.resize(256, 256)
        r.set_layout(1)
        r.render(frames=3)
        img = r.read_display()
        assert img.shape == (256, 256, 4)
        r.close()

    cycle(0)
    gc.collect(); torch.cuda.synchronize()
    free0 = torch.cuda.mem_get_info()[0]
    for i in range(1, 21):
        cycle(i)
    gc.collect(); torch.cuda.synchronize()
    free1 = torch.cuda.mem_get_info()[0]
    assert free0 - free1 < 64 << 20, (free0 - free1) / 2 ** 20


def test_bench_two_ranks_rehearsal_gathers_the_one_rank_image():
    """bench.py's N > 1 path end to end on the one GPU there is: `--gpus 2 --rehearse-gloo` starts two ranks (child processes
    of bench.py's own launcher) that share the device and use the gloo backend -- tile dealing in the balanced order, sharded
    contexts, 64-frame launches, snapshot + all_gather + de-tile, the reductions of the JSON line: everything but RCCL.  The
    gathered image of its 96 accumulation frames must be the image a single rank gathers (`--force-gather`) bit for bit, the
    sample counts must agree, and the line must say n_gpus 2 and call itself a rehearsal."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    lean = ["--steps", "2", "--warmup", "1", "--no-cpu-baseline", "--no-mode-variants", "--no-skip-variant",
            "--no-side-measurements"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}

    def run(extra):
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *extra, *lean], env=env, capture_output=True,
                           text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-500:]
        return json.loads(lines[0])

    one = run(["--gpus", "1", "--force-gather"])
    two = run(["--gpus", "2", "--rehearse-gloo"])
    assert one["n_gpus"] == 1 and two["n_gpus"] == 2 and two["rehearsal"] and not one["rehearsal"]
    assert one["config"]["image_sha256"] and one["config"]["image_sha256"] == two["config"]["image_sha256"]
    assert one["config"]["samples_per_frame"] == two["config"]["samples_per_frame"]
    assert two["config"]["frames_per_launch"] == 64 and one["config"]["frames_per_launch"] == 32
    assert two["config"]["gathers"] >= 2 and "image-tiles x2" in two["config"]["parallelism"]
    assert two["cpu_baseline"] is None and two["scaling"] == "strong"


def test_bench_dump_outputs_repeat_bit_for_bit(tmp_path):
    """`bench.py --dump-outputs DIR` on a small scene, twice with the same arguments: exactly --steps timed steps, a
    ms_per_step in the line, and the dumped image and counters of the timed run identical from run to run (the inputs
    are seeded); the image is the accumulated mean of the warm-up and timed frames, finite and not blank."""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    args = ["--gpus", "1", "--steps", "3", "--warmup", "1", "--frames-per-step", "8", "--volume", "64", "--width", "320",
            "--height", "192", "--no-cpu-baseline", "--no-mode-variants", "--no-skip-variant", "--no-side-measurements"]
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    dumps = []
    for i in range(2):
        out = tmp_path / f"run{i}"
        p = subprocess.run([sys.executable, os.path.join(root, "bench.py"), *args, "--dump-outputs", str(out)], env=env,
                           capture_output=True, text=True, timeout=600)
        assert p.returncode == 0, p.stderr[-2000:]
        lines = [ln for ln in p.stdout.splitlines() if ln.startswith("{")]
        assert len(lines) == 1, p.stdout[-500:]
        line = json.loads(lines[0])
        assert line["steps"] == 3 and line["config"]["frames_timed"] == 24 and line["ms_per_step"] > 0
        dumps.append({f.name: np.load(f) for f in out.iterdir()})
    assert sorted(dumps[0]) == ["accum.npy", "counters.npy"]
    img, cnt = dumps[0]["accum.npy"], dumps[0]["counters.npy"]
    assert img.shape == (192, 320, 4) and img.dtype == np.float32 and np.isfinite(img).all() and img.max() > 0
    assert cnt[2] == 24 and cnt[0] > 0                       # the counters cover the 24 timed frames
    for name in dumps[0]:
        assert np.array_equal(dumps[0][name], dumps[1][name]), name
