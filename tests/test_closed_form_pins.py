"""Closed-form pins for shadowed DVR, the intensity projections and the slices.

tests/shadow_ref.py, tests/projection_ref.py and tests/slice_ref.py restate the kernels in NumPy and the GPU tests hold the device
to them bit for bit; an error the kernel and its restatement share passes those tests.  Here every pin has two legs -- the
restatement (CPU) and the device (`gpu`, no restatement in between) -- and both are held to answers computed in float64 from the
scene alone (tests/closed_form.py: spacing and extent, camera position / look-at / fov, the clip box, the light, the TF entries).
Every tolerance is derived in its test's docstring, and every pin has a negative control: a committed CPU assertion that a
deliberately wrong float64 answer (light sign flipped, positions shifted, image mirrored, the old clip clamp ...) lies outside the
same tolerance."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import closed_form as CF
from tests import common

F32 = np.float32
EPS32 = 2.0 ** -24                      # unit roundoff of binary32
LAYOUTS = {k: common.LAYOUTS[k] for k in ("brickf32", "bricku8", "reference", "cellquad")}


def _normalised(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _renderer(g, w, h, layout, tf, L):
    from volxel_amd import Volxel3DRenderer
    r = Volxel3DRenderer(w, h, layout=layout)
    r.setup_from_grid(g)
    r.change_transfer_func(tf, L)
    return r


def _set_params(r, p):
    r._check(r._lib.vx_set_params(r._ctx, C.byref(p)))


# ==== 1. shadowed DVR against the single-scatter integral ===========================================================
SH_W, SH_H = 24, 16
ALPHA, COLOUR = 0.1, np.array([0.8, 0.5, 0.3])
STEP = 0.125                                                   # dvr_step_voxels
EXT = (64, 64, 64)                                             # a 32^3 stack pads to 64^3 index positions
CLIP = ((4 / 64, 6 / 64, 3 / 64), (27 / 64, 21 / 64, 29 / 64))  # off-centre, not a cube, inside the data with its taps
ERT_EPS = 1e-4                                                 # dvr_ert_epsilon: exp(-ert_tau)
K = 0.9 * (1.0 / (4.0 * math.pi)) * 4.01                       # albedo * f_p * Le (fragment.frag:94-97, no environment)
SH_LIGHTS = {"axis": (0.0, -1.0, 0.0), "diagonal": tuple(_normalised((-1, -1, -1))),
             "oblique": tuple(_normalised((0.3, -0.8, 0.5)))}
SPACINGS = {"iso": (1.0, 1.0, 1.0), "aniso": (0.5, 1.0, 2.0)}


class ShadowScene:
    """The homogeneous scene in float64: extinction sigma = alpha * volume_maj per world unit, volume_maj = S (the longest side
    of the grid's box, the normalisation's density scale), the clip box, the camera looking at its centre, the light grid's
    nodes and their exact transmittance T(x) = exp(-sigma * chord(x, -light))."""

    def __init__(self, light, stride, spacing):
        self.light = np.asarray(light, float)
        self.w = -self.light                                   # toward the light (w_i = -light_dir)
        self.stride, self.spacing = stride, np.asarray(spacing, float)
        self.sigma = ALPHA * CF.world_scale(EXT, spacing)
        self.lo, self.hi = CF.world_box(EXT, spacing, *CLIP)
        self.box_idx = (np.asarray(CLIP[0]) * 64.0, np.asarray(CLIP[1]) * 64.0)
        self.look = 0.5 * (self.lo + self.hi)
        self.eye = self.look + np.array([0.37, 0.27, -0.38])
        self.ipw = CF.index_per_world(spacing, EXT)
        self.dt_light = STEP / np.linalg.norm(self.w * self.ipw)          # world units per light-march step
        s = stride
        self.n = [(e - 1 + s - 1) // s + 1 for e in EXT]
        k, j, i = np.meshgrid(*[np.arange(m) for m in self.n[::-1]], indexing="ij")
        self.node_idx = np.stack([s * i + 0.5, s * j + 0.5, s * k + 0.5], axis=-1)
        self.node_world = CF.index_to_world(self.node_idx, EXT, spacing)
        self.T_nodes = self.transmittance(self.node_world)
        lo, hi = self.box_idx
        self.inside = ((self.node_idx >= lo) & (self.node_idx <= hi)).all(axis=-1)
        # the first and last node inside the box per axis (the clamp of the look-up)
        self.node_lo = [int(math.ceil((lo[a] - 0.5) / s)) for a in range(3)]
        self.node_hi = [int(math.floor((hi[a] - 0.5) / s)) for a in range(3)]
        # light-march bound: |n dt_L - s| <= dt_L / 2 and |d exp(-sigma s) / ds| <= sigma; fp32: at most n_max roundings of tau
        # (each <= 2^-24 tau, and tau exp(-tau) <= 1/e) and exp itself (a few ulp)
        n_max = float(CF.chord(self.node_world, self.w, self.lo, self.hi).max()) / self.dt_light + 2.0
        self.e_light = self.sigma * self.dt_light / 2.0 + n_max * EPS32 + 4 * EPS32
        # the light march's own answer: a node inside the box takes m = ceil(s / dt_L - 1/2) samples of alpha maj dt_L = sigma dt_L
        # each, T_q = exp(-sigma dt_L m).  fp32 moves s / dt_L by far less than 1e-2 (relative errors of a few 2^-24 on at most
        # ~10^3), so m is certain unless s / dt_L - 1/2 lies within 1e-2 of an integer; there one sample either way: sigma dt_L.
        x = CF.chord(self.node_world, self.w, self.lo, self.hi) / self.dt_light - 0.5
        self.T_q = np.exp(-self.sigma * self.dt_light * np.maximum(np.ceil(x), 0.0))
        ambiguous = np.abs(x - np.round(x)) < 1e-2
        self.e_q = np.where(ambiguous, self.sigma * self.dt_light, 0.0) + n_max * EPS32 + 4 * EPS32

    def transmittance(self, x, w=None):
        return np.exp(-self.sigma * CF.chord(x, self.w if w is None else w, self.lo, self.hi))

    def rays(self):
        (d,), _ = CF.camera_rays(self.eye, self.look, SH_W, SH_H)
        near, far = CF.slab(self.eye, d, self.lo, self.hi)
        return d, near, far

    def integral(self, w=None):
        """colour-free image / K: Int_near^far sigma exp(-sigma (t - near)) exp(-sigma s(t)) dt, exactly.  s(t), the distance from
        the ray point to the box exit toward the light, is the minimum over the axes with w_a != 0 of (b_a - x_a(t)) / w_a, an
        affine function of t per axis: the integrand is exp(affine) between the break points where the minimising axis changes."""
        w = self.w if w is None else np.asarray(w, float)
        d, near, far = self.rays()
        far = np.maximum(far, near)
        act = [a for a in range(3) if w[a] != 0.0]
        b = np.where(w > 0, self.hi, self.lo)
        alpha = {a: (b[a] - self.eye[a]) / w[a] for a in act}            # s_a(t) = alpha_a + beta_a t
        beta = {a: -d[..., a] / w[a] for a in act}
        cuts = [near, far]
        for ia, a in enumerate(act):
            for c in act[ia + 1:]:
                with np.errstate(divide="ignore", invalid="ignore"):
                    t = (alpha[c] - alpha[a]) / (beta[a] - beta[c])
                cuts.append(np.clip(np.where(np.isfinite(t), t, near), near, far))
        ts = np.sort(np.stack(cuts, axis=-1), axis=-1)
        total = np.zeros(near.shape)
        for m in range(ts.shape[-1] - 1):
            ta, tb = ts[..., m], ts[..., m + 1]
            mid = 0.5 * (ta + tb)
            s_mid = np.stack([alpha[a] + beta[a] * mid for a in act], axis=-1)
            pick = np.argmin(s_mid, axis=-1)
            al = np.choose(pick, [np.broadcast_to(alpha[a], near.shape) for a in act])
            be = np.choose(pick, [beta[a] for a in act])
            kk = -self.sigma * (1.0 + be)
            span = tb - ta
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                e0 = np.exp(np.where(span > 0, -self.sigma * (ta - near) - self.sigma * (al + be * ta), -np.inf))
                part = np.where(np.abs(kk * span) > 1e-12, np.expm1(kk * span) / kk, span)
            total += np.where(span > 0, self.sigma * e0 * part, 0.0)
        return total

    def samples(self, d, near, far):
        """the march contract's samples in float64: dt = step / |idir|, n = ceil((l - dt/2) / dt), t_k = near + (k + 1/2) dt"""
        dt = STEP / np.linalg.norm(d * self.ipw, axis=-1)
        x = (far - near - 0.5 * dt) / dt
        n = np.where(x > 0, np.ceil(x), 0).astype(np.int64)
        kk = np.arange(max(int(n.max()), 1))
        valid = kk < n[..., None]
        t = near[..., None] + (kk + 0.5) * dt[..., None]
        pos = self.eye + t[..., None] * d[..., None, :]
        dT = np.where(valid, np.exp(-self.sigma * kk * dt[..., None]) - np.exp(-self.sigma * (kk + 1) * dt[..., None]), 0.0)
        return dt, x, n, valid, pos, dT

    def interp_nodes(self, pos, clamp=None, table=None, shift=0.0):
        """the 8 light-grid nodes the look-up of the cell-frame position of pos blends (DESIGN: g = q / s clamped per axis to
        [node_lo, node_hi], cell min(floor(g), n - 2)); clamp = (lo, hi) lists to replace the clamp, table = the node values
        (default T_nodes), shift = voxels added to q (negative controls).  Returns (8 node values, 8 trilinear weights)"""
        table = self.T_nodes if table is None else table
        q = CF.world_to_index(pos, EXT, self.spacing) - 0.5 + shift
        lo, hi = clamp if clamp is not None else (self.node_lo, self.node_hi)
        cells, fr = [], []
        for a in range(3):
            g = np.clip(q[..., a] / self.stride, lo[a], hi[a])
            c = np.minimum(np.floor(g), self.n[a] - 2)
            cells.append(c.astype(np.int64))
            fr.append(g - c)
        vals, wts = [], []
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    vals.append(table[cells[2] + dz, cells[1] + dy, cells[0] + dx])
                    wts.append((fr[0] if dx else 1 - fr[0]) * (fr[1] if dy else 1 - fr[1]) * (fr[2] if dz else 1 - fr[2]))
        return np.stack(vals, axis=-1), np.stack(wts, axis=-1)

    def bounds(self, first_only=False):
        """(lower, upper) of (image / K - integral) per pixel and colour channel; first_only: a march that ends at its first
        contributing sample (dvr_ert_tau <= 0), compared with its own closed form dT_0 T(x_0) (see test_shadowed_image)"""
        d, near, far = self.rays()
        dt, x, n, valid, pos, dT = self.samples(d, near, far)
        if first_only:
            valid = valid & (np.arange(valid.shape[-1]) == 0)
            dT = np.where(valid, dT, 0.0)
        T_k = self.transmittance(pos)
        vals, _ = self.interp_nodes(pos)
        d_hi = (dT * (vals.max(axis=-1) - T_k)).sum(axis=-1)
        d_lo = (dT * (vals.min(axis=-1) - T_k)).sum(axis=-1)
        if first_only:
            common = dT[..., 0] * self.e_light + 2e-4
        else:
            act = self.w != 0
            lip_s = np.abs(d[..., act] / self.w[act]).max(axis=-1)       # |ds/dt| along the ray: s is a min of affine functions
            near_int = np.abs(x - np.round(x)) < 1e-3                      # fp32 may take one sample more or less there
            common = (self.sigma * dt / 2 * (1.0 + lip_s) + near_int * self.sigma * dt + dT.sum(axis=-1) * self.e_light
                      + 2e-4 + ERT_EPS)
        return (d_lo - common), (d_hi + common)

    def march_model(self, first_only=False, shift=0.0):
        """(model, tol) per pixel in units of K colour: the march contract evaluated in float64 on the closed-form rays, each
        sample's dT_k times the contracted look-up (clamp, lattice, trilinear weights) of the light march's own node values T_q.
        The device differs from it by: the node values, sum_k dT_k sum_n w_n e_q(n); one sample of sigma dt where fp32 may round
        n the other way; fp32 positions (a few 1e-5 voxel: the weights move by that over the stride, < 1e-4 of a node
        difference); 2e-4 of fp32 compositing as in test_analytic_pins; early termination exp(-ert_tau)."""
        d, near, far = self.rays()
        dt, x, n, valid, pos, dT = self.samples(d, near, far)
        if first_only:
            dT = np.where(np.arange(dT.shape[-1]) == 0, dT, 0.0)
        vals, wts = self.interp_nodes(pos, table=self.T_q, shift=shift)
        evals, _ = self.interp_nodes(pos, table=self.e_q, shift=shift)
        model = (dT * (vals * wts).sum(axis=-1)).sum(axis=-1)
        tol = (dT * (evals * wts).sum(axis=-1)).sum(axis=-1) + 1e-4 + 2e-4
        if not first_only:
            tol = tol + (np.abs(x - np.round(x)) < 1e-3) * self.sigma * dt + ERT_EPS
        return model, tol

    def first_sample(self):
        d, near, far = self.rays()
        dt, x, n, valid, pos, dT = self.samples(d, near, far)
        return np.where(valid[..., 0], dT[..., 0] * self.transmittance(pos[..., 0, :]), 0.0)

    def tf(self, L=16):
        return np.tile(np.array([*COLOUR, ALPHA], dtype=np.float32), (L, 1)).reshape(-1)

    def params(self, oracle, g, L=16, ert_eps=ERT_EPS):
        _, _, _, _, p = CF.make_pin_scene(g, SH_W, SH_H, "dvr", self.eye, self.look, CLIP[0], CLIP[1], self.light,
                                          dvr_step_voxels=STEP, dvr_shadow_stride=self.stride, dvr_jitter=False,
                                          dvr_ert_epsilon=ert_eps, max_samples=1 << 20)
        return p

    def check_grid(self, got):
        err = np.abs(got.astype(np.float64) - self.T_nodes)[self.inside]
        assert self.inside.sum() >= 8 and float(self.T_nodes[self.inside].min()) < 0.3
        assert float(err.max()) <= self.e_light, (float(err.max()), self.e_light)
        err_q = np.abs(got.astype(np.float64) - self.T_q)[self.inside]
        assert (err_q <= self.e_q[self.inside]).all(), float((err_q / self.e_q[self.inside]).max())
        return float(err.max()) / self.e_light

    def check_image(self, img, first_only=False):
        want = self.first_sample() if first_only else self.integral()
        lo, hi = self.bounds(first_only)
        err = img[..., :3].astype(np.float64) / (K * COLOUR) - want[..., None]
        assert float(want.max()) > (0.005 if first_only else 0.3)
        ok = (err >= lo[..., None]) & (err <= hi[..., None])
        assert ok.all(), (int((~ok).sum()), float(np.abs(err).max()))
        # the tight statement: the march contract's float64 model (march_model), per pixel
        model, tol = self.march_model(first_only)
        e_m = np.abs(img[..., :3].astype(np.float64) / (K * COLOUR) - model[..., None])
        assert (e_m <= tol[..., None]).all(), float((e_m / tol[..., None]).max())
        self.model_margin = float((e_m / tol[..., None]).max())
        mid, half = 0.5 * (hi + lo)[..., None], 0.5 * (hi - lo)[..., None]
        return float((np.abs(err - mid) / half).max())          # observed / allowed, <= 1


_SHADOW_CASES = [(l, s, sp) for l in sorted(SH_LIGHTS) for s in (1, 2, 4) for sp in sorted(SPACINGS)]


@pytest.fixture(scope="module")
def shadow_grids():
    from oracle import oracle as O
    return {k: CF.homogeneous_grid(O, spacing=v) for k, v in SPACINGS.items()}


def test_shadow_scene_geometry_is_hand_derived():
    """the hand-written world map equals scene.Volume.normalise's in float64, and the homogeneous medium's sigma is volume_maj * alpha"""
    from volxel_amd.scene import Grid, Volume
    for sp in SPACINGS.values():
        vol = Volume(Grid((0.0, 1.0), np.asarray(EXT, float), np.diag([*sp, 1.0])))
        S = vol.normalise()
        M = vol.combined_transform()
        idx = np.array([[0, 0, 0], [64, 64, 64], [3.5, 17.25, 40.0]], float)
        assert np.allclose((M @ np.c_[idx, np.ones(3)].T).T[:, :3], CF.index_to_world(idx, EXT, sp), rtol=0, atol=1e-15)
        assert S == CF.world_scale(EXT, sp)


@pytest.mark.parametrize("light,stride,spacing", _SHADOW_CASES)
def test_shadow_restatement_meets_closed_form(shadow_grids, light, stride, spacing):
    """CPU leg of pin 1 (shadow_ref.light_grid / dvr_image_shadowed against float64).

    Light grid: node (i, j, k) sits at index position s (i, j, k) + 1/2; inside the clip box its march covers n dt_L with
    |n dt_L - s(node)| <= dt_L / 2 (t0 = dt_L / 2, n = ceil((s - t0) / dt_L)), so |T_L - exp(-sigma s)| <= sigma dt_L / 2, plus
    fp32: n roundings of tau of at most 2^-24 tau each, tau exp(-tau) <= 1/e, and exp (ShadowScene.e_light).

    Image (per pixel, per channel, in units of K colour): the march has samples t_k = near + (k + 1/2) dt, k < n, each adds
    dT_k G_k with dT_k = exp(-sigma k dt) - exp(-sigma (k + 1) dt) and G_k the light grid's trilinear -- a convex combination of
    8 node values, each within e_light of T at its node.  Against the integral:
      * Beer-Lambert: the intervals [k dt, (k + 1) dt] cover n dt, within dt / 2 of the chord: sigma dt / 2;
      * inside interval k, |T(x(t)) - T(x_k)| <= sigma |ds/dt| dt / 2, |ds/dt| <= max_a |d_a / w_a| (s is a min of affine functions);
      * the light grid: e_light times sum dT_k;
      * the interpolation: sum_k dT_k (min or max over the 8 clamped nodes of T(node) - T(x_k)), computed in float64;
      * fp32: 2e-4 (as test_analytic_pins), early termination exp(-ert_tau) = 1e-4, and one more sample of sigma dt where
        (l - dt/2) / dt lies within 1e-3 of an integer (fp32 may round n the other way).
    The signed interpolation term makes the bound two-sided.  That bound is wide where the light grid varies over a node
    spacing (a look-up off by half a voxel or half a node stays inside it); ShadowScene.march_model is the tight statement
    beside it: the contract's march and look-up in float64 over the light march's own node values, within about 3e-4 where no
    sample count or node is ambiguous -- the light grid is checked against those node values too (e_q)."""
    from oracle import oracle as O
    from tests import shadow_ref as SR
    sc = ShadowScene(SH_LIGHTS[light], stride, SPACINGS[spacing])
    g = shadow_grids[spacing]
    p = sc.params(O, g)
    tf = sc.tf()
    T, _ = SR.light_grid(p, g, tf, 16, stride)
    sc.check_grid(T)
    img, _, _ = SR.dvr_image_shadowed(p, g, tf, 16, T, stride)
    sc.check_image(img)


def test_shadow_negative_controls():
    """the wrong float64 answers lie outside the bounds of test_shadow_restatement_meets_closed_form:
      * light grid: the light's sign flipped (+light_dir), the nodes shifted by half a voxel (at s i instead of s i + 1/2), and on
        anisotropic voxels the light direction mapped by density_transform instead of its inverse;
      * light grid against the march's own node values T_q: every case's nodes shifted by half a node;
      * image: the light's sign flipped; plain DVR (T_L = 1); the DESIGN's earlier [0, n - 1] clamp of the look-up (outside nodes
        whose march misses the box read 1): a float64 model of the march with that clamp; and in every case the look-up shifted by
        half a voxel and by half a node, against march_model's bound (twice it: the model's tolerance is on both sides)."""
    sc = ShadowScene(SH_LIGHTS["oblique"], 2, SPACINGS["aniso"])
    ins = sc.inside
    flipped = sc.transmittance(sc.node_world, w=-sc.w)
    assert np.abs(flipped - sc.T_nodes)[ins].max() > 5 * sc.e_light
    shifted = sc.transmittance(CF.index_to_world(sc.node_idx - 0.5, EXT, sc.spacing))
    assert np.abs(shifted - sc.T_nodes)[ins].max() > 2 * sc.e_light
    w_wrong = _normalised(sc.w * sc.spacing ** 2)
    wrong_map = sc.transmittance(sc.node_world, w=w_wrong)
    assert np.abs(wrong_map - sc.T_nodes)[ins].max() > 5 * sc.e_light

    for light, stride, spacing in (("oblique", 2, "aniso"), ("diagonal", 1, "iso"), ("axis", 4, "iso")):
        sc = ShadowScene(SH_LIGHTS[light], stride, SPACINGS[spacing])
        want = sc.integral()
        lo, hi = sc.bounds()

        def outside(model):
            e = model - want
            return bool(((e < lo) | (e > hi)).any())

        assert outside(sc.integral(w=-sc.w)), light
        d, near, far = sc.rays()
        assert outside(1.0 - np.exp(-sc.sigma * np.maximum(far - near, 0.0))), light
    # the light grid's nodes half a node off, against the light march's own values
    for light, stride, spacing in _SHADOW_CASES:
        sc = ShadowScene(SH_LIGHTS[light], stride, SPACINGS[spacing])
        shifted = sc.transmittance(CF.index_to_world(sc.node_idx - 0.5 * stride, EXT, sc.spacing))
        assert (np.abs(shifted - sc.T_q) > sc.e_q)[sc.inside].any(), (light, stride, spacing)
        # the look-up half a voxel or half a node off breaks the per-pixel model bound in every case
        model, tol = sc.march_model()
        for shift in {0.5, 0.5 * stride}:
            wrong, _ = sc.march_model(shift=shift)
            assert (np.abs(wrong - model) > 2 * tol).any(), (light, stride, spacing, shift)
    # the [0, n - 1] clamp: with the light along -y, nodes beyond the box's x and z faces see no box (T = 1)
    sc = ShadowScene(SH_LIGHTS["axis"], 4, SPACINGS["iso"])
    d, near, far = sc.rays()
    dt, x, n, valid, pos, dT = sc.samples(d, near, far)
    vals, wts = sc.interp_nodes(pos, clamp=([0, 0, 0], [m - 1 for m in sc.n]))
    model = (dT * (vals * wts).sum(axis=-1)).sum(axis=-1)
    lo, hi = sc.bounds()
    e = model - sc.integral()
    assert ((e < lo) | (e > hi)).any()
    vals, wts = sc.interp_nodes(pos)                      # and the contracted clamp's model lies inside
    e = (dT * (vals * wts).sum(axis=-1)).sum(axis=-1) - sc.integral()
    assert ((e >= lo) & (e <= hi)).all()


SH_ROUTES = {"lds_brickf32": ("brickf32", 16, ERT_EPS), "lds_bricku8": ("bricku8", 16, ERT_EPS),
             "generic_reference": ("reference", 16, ERT_EPS), "generic_cellquad": ("cellquad", 16, ERT_EPS),
             "generic_long_tf": ("brickf32", 4096, ERT_EPS), "generic_ert0": ("brickf32", 16, 2.0)}


@pytest.mark.gpu
@pytest.mark.parametrize("light,stride,spacing", _SHADOW_CASES)
def test_shadowed_image(shadow_grids, light, stride, spacing):
    """GPU leg of pin 1: the device's light grid and image against the float64 answers with the bounds of
    test_shadow_restatement_meets_closed_form, on both kernels: render_dvr_lds_shadow (brickf32 / bricku8, dvr_ert_tau > 0) and
    render_generic_shadow (reference and cellquad layouts; a TF of 4096 > TF_LDS_MAX entries; dvr_ert_tau <= 0).  With
    dvr_ert_tau <= 0 (an epsilon >= 1) every ray ends at its first contributing sample: the image is dT_0 G_0 against
    dT_0 T(x_0), bound dT_0 (e_light + the interpolation term) + 2e-4."""
    from oracle import oracle as O
    sc = ShadowScene(SH_LIGHTS[light], stride, SPACINGS[spacing])
    g = shadow_grids[spacing]
    margins = {}
    for route, (layout, L, eps) in SH_ROUTES.items():
        p = sc.params(O, g, L=L, ert_eps=eps)
        r = _renderer(g, SH_W, SH_H, LAYOUTS[layout], sc.tf(L), L)
        try:
            _set_params(r, p)
            r._check(r._lib.vx_render_frame(r._ctx, 0, 0.0))
            img = r.read_accum()
            grid = r.read_shadow_grid()
            lds = r.counters().lds_reads
            # the route: the LDS-window kernel counts its LDS tap reads, render_generic_shadow reads no LDS taps
            assert (lds > 0) == route.startswith("lds_"), (route, lds)
        finally:
            r.close()
        margins[route] = (sc.check_grid(grid), sc.check_image(img, first_only=eps >= 1.0), sc.model_margin)
    print("margins", light, stride, spacing, margins)


# ==== 2. MIP / MinIP against a float64 continuous max / min ===========================================================
PJ_W, PJ_H = 40, 28
PJ_STEP = 0.25                                                  # dvr_step_voxels
PJ_FINE = 0.02                                                  # the float64 march, in voxels along the ray
PJ_CLIP = ((2 / 64, 2 / 64, 2 / 64), (28 / 64, 24 / 64, 19 / 64))   # inside the 30 x 26 x 21 data, taps included
PJ_SR = (0.42, 1.5)                                             # sample_range: some minima (and maxima) fall below it


def _projection_voxels():
    """a ragged 30 x 26 x 21 stack (x, y, z): a ramp, an off-centre Gaussian blob and an off-centre dip, so that the maximum and
    the minimum of most rays lie inside the ray rather than at an end"""
    z, y, x = np.meshgrid(np.arange(21), np.arange(26), np.arange(30), indexing="ij")
    ramp = 900.0 + 30.0 * x + 22.0 * y + 14.0 * z
    blob = 1800.0 * np.exp(-((x - 19.0) ** 2 + (y - 9.0) ** 2 + (z - 12.0) ** 2) / (2 * 3.5 ** 2))
    dip = 900.0 * np.exp(-((x - 8.0) ** 2 + (y - 15.0) ** 2 + (z - 7.0) ** 2) / (2 * 3.0 ** 2))
    return np.round(ramp + blob - dip).astype(np.uint16)


class ProjectionScene:
    """rays of the closed-form camera through the clip box, the decoded voxels, a float64 march at PJ_FINE voxels"""

    def __init__(self, oracle):
        self.grid = oracle.BrickGrid(_projection_voxels(), (1.0, 1.0, 1.0))
        self.ext = tuple(int(e) for e in self.grid.index_extent)
        self.dec = CF.decode(oracle, self.grid)
        self.lo, self.hi = CF.world_box(self.ext, (1, 1, 1), *PJ_CLIP)
        self.look = 0.5 * (self.lo + self.hi) + np.array([0.01, -0.02, 0.0])
        self.eye = self.look + np.array([0.28, 0.22, -0.5])
        self.ipw = CF.index_per_world((1, 1, 1), self.ext)
        (self.d,), _ = CF.camera_rays(self.eye, self.look, PJ_W, PJ_H)
        self.near, self.far = CF.slab(self.eye, self.d, self.lo, self.hi)
        # per cell (cell-frame floor c, taps c and c + 1; c from -2) and axis: the largest difference of the cell's 4 voxel
        # pairs along that axis -- the trilinear is that Lipschitz along the axis inside the cell -- then the maximum over the
        # cell and its 26 neighbours, so that a cell the ray crosses between two float64 samples (0.02 voxel apart) is covered
        P = np.pad(self.dec, 2)
        gs = []
        for ax in (2, 1, 0):                                                 # x, y, z of the (z, y, x) array
            D = np.abs(np.diff(P, axis=ax))
            for other in (0, 1, 2):
                if other != ax:
                    D = np.maximum(np.take(D, range(D.shape[other] - 1), axis=other),
                                   np.take(D, range(1, D.shape[other]), axis=other))
            gs.append(D[:P.shape[0] - 1, :P.shape[1] - 1, :P.shape[2] - 1])
        self.g_cell = [self._dilate(g) for g in gs]
        self.g = np.array([g.max() for g in self.g_cell])

    @staticmethod
    def _dilate(g):
        out = g.copy()
        for ax in range(3):
            pad = np.pad(out, [(1, 1) if a == ax else (0, 0) for a in range(3)], mode="edge")
            out = np.maximum(np.maximum(np.take(pad, range(0, g.shape[ax]), axis=ax), np.take(pad, range(1, g.shape[ax] + 1), axis=ax)),
                             np.take(pad, range(2, g.shape[ax] + 2), axis=ax))
        return out

    def extrema(self, shift=0.0):
        """float64 (max, min) of the trilinear along each ray over [near, far], endpoints included; shift moves the positions by
        that many voxels (negative control)"""
        ilen = np.linalg.norm(self.d * self.ipw, axis=-1)                   # voxels per world unit along the ray
        chord = np.maximum(self.far - self.near, 0.0)
        J = int(np.ceil((chord * ilen).max() / PJ_FINE)) + 1
        u = np.linspace(0.0, 1.0, J)
        t = self.near[..., None] + chord[..., None] * u
        pos = self.eye + t[..., None] * self.d[..., None, :]
        q = CF.world_to_index(pos, self.ext, (1, 1, 1)) - 0.5 + shift
        v = CF.trilinear(self.dec, q[..., 0], q[..., 1], q[..., 2])
        # the ray's Lipschitz constant per world unit: the largest sum_a |idir_a| g_a over the cells its samples lie in
        idir = np.abs(self.d * self.ipw)
        lip = np.zeros(q.shape[:-1])
        for a in range(3):
            c = [np.clip(np.floor(q[..., b]).astype(np.int64) + 2, 0, self.g_cell[a].shape[2 - b] - 1) for b in range(3)]
            lip = lip + idir[..., a, None] * self.g_cell[a][c[2], c[1], c[0]]
        self.lip = lip.max(axis=-1)
        return v.max(axis=-1), v.min(axis=-1), chord * ilen / max(J - 1, 1)

    def bound(self, h_fine):
        """Lip (dt + dt_fine) + rounding per pixel, in density units (Lip per ray, from extrema)"""
        idir = self.d * self.ipw
        lip = self.lip
        dt = PJ_STEP / np.linalg.norm(idir, axis=-1)
        h = h_fine / np.linalg.norm(idir, axis=-1)
        rounding = 8 * EPS32 * float(max(self.ext)) * float(self.g.sum()) + 16 * EPS32
        return lip * (dt + h) + rounding

    def params(self, mode, L, **kw):
        _, _, _, _, p = CF.make_pin_scene(self.grid, PJ_W, PJ_H, mode, self.eye, self.look, PJ_CLIP[0], PJ_CLIP[1],
                                          (0.0, -1.0, 0.0), dvr_step_voxels=PJ_STEP, sample_range=PJ_SR,
                                          max_samples=1 << 20, **kw)
        return p


def _readback_tf(L):
    """r = g = b = (i + 1/2) / L, alpha 1: the pixel shows its bin's centre, within 1 / (2L) of m under floor(m L)"""
    c = (np.arange(L) + 0.5) / L
    return np.stack([c, c, c, np.ones(L)], axis=-1).astype(np.float32).reshape(-1)


def _check_projection(img, want, tol, chord_vox, L, hit):
    """every missing ray is (0, 0, 0, 1); a ray whose m lies below sample_range[0] by more than tol is black; every other ray
    away from the threshold shows m within tol + 1 / (2L) in r, g and b (rays under 2 samples long are skipped)"""
    miss = ~hit
    assert np.array_equal(img[miss], np.tile(np.array([0, 0, 0, 1], np.float32), (int(miss.sum()), 1)))
    long_enough = hit & (chord_vox >= 2 * PJ_STEP)
    below = long_enough & (want < PJ_SR[0] - tol)
    above = long_enough & (want > PJ_SR[0] + tol)
    assert below.sum() >= 10 and above.sum() >= 100 and miss.sum() >= 10
    assert (img[below][:, :3] == 0).all()
    allowed = tol + 1.0 / (2 * L) + 4 * EPS32
    err = np.abs(img[..., :3].astype(np.float64) - want[..., None])[above]
    assert (err <= allowed[above][:, None]).all(), float(err.max())
    return float((err / allowed[above][:, None]).max())


@pytest.fixture(scope="module")
def proj_scene():
    from oracle import oracle as O
    return ProjectionScene(O)


def _proj_truth(sc):
    mx, mn, h = sc.extrema()
    return {"mip": mx, "minip": mn}, sc.bound(PJ_FINE), sc.far > sc.near


def test_projection_reference_march_agrees_with_scipy(proj_scene):
    """the float64 trilinear of the decoded voxels against scipy.ndimage.map_coordinates (order 1, zero padding)"""
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(5)
    q = rng.uniform(-2.0, 34.0, size=(500, 3))
    want = ndimage.map_coordinates(proj_scene.dec, [q[:, 2], q[:, 1], q[:, 0]], order=1, mode="grid-constant", cval=0.0)
    assert np.abs(CF.trilinear(proj_scene.dec, q[:, 0], q[:, 1], q[:, 2]) - want).max() <= 1e-12


@pytest.mark.parametrize("L", [8, 1024, 4096])
@pytest.mark.parametrize("mode", ["mip", "minip"])
def test_projection_restatement_meets_closed_form(proj_scene, mode, L):
    """CPU leg of pin 2 (projection_ref.projection_image against float64).  The float64 answer m* marches the closed-form ray
    through the clip box at PJ_FINE voxels with the endpoints, so it is within Lip dt_fine / 2 of the continuous max / min; the
    kernel's samples are dt apart and within dt of either end (with jitter off the start offset is 1/2), so its max / min is
    within Lip dt of the continuous one.  Lip per world unit along the ray: the largest sum_a |idir_a| g_a over the cells the
    ray crosses, g_a a cell's largest voxel difference along axis a (the trilinear is g_a-Lipschitz along a inside the cell),
    taken over the cell and its neighbours (ProjectionScene).  L = 8 makes the read-back bins (1/16) wider than that bound, so
    the floor(m L) bin rule itself is pinned (test_projection_negative_controls: the round(m L) rule breaks it).  fp32: sample positions within
    8 * 2^-24 * 64 voxels (|q| <= 64), densities within 16 * 2^-24.  The read-back TF adds 1 / (2L) (floor(m L) bins)."""
    from tests import projection_ref as PR
    sc = proj_scene
    truth, tol, hit = _proj_truth(sc)
    p = sc.params(mode, L)
    img, _, _, _ = PR.projection_image(p, sc.grid, _readback_tf(L), L, minip=mode == "minip")
    chord_vox = np.maximum(sc.far - sc.near, 0) * np.linalg.norm(sc.d * sc.ipw, axis=-1)
    _check_projection(img, truth[mode], tol, chord_vox, L, hit)


def test_projection_negative_controls(proj_scene):
    """outside the same tolerance: the image mirrored left-right, MIP and MinIP swapped, the positions shifted by half a voxel, and at L = 8 the TF bin picked by
    round(m L) instead of floor(m L)"""
    sc = proj_scene
    truth, tol, hit = _proj_truth(sc)
    ok = hit & (np.maximum(sc.far - sc.near, 0) * np.linalg.norm(sc.d * sc.ipw, axis=-1) >= 2 * PJ_STEP)
    ok = ok & ok[:, ::-1]
    allowed = tol + 1.0 / (2 * 4096)
    for m in ("mip", "minip"):
        assert (np.abs(truth[m][:, ::-1] - truth[m]) > allowed)[ok].any(), m
    assert (np.abs(truth["mip"] - truth["minip"]) > allowed)[ok].any()
    mx, mn, _ = sc.extrema(shift=0.5)
    sc.extrema()                                                            # restore sc.lip
    assert (np.abs(mx - truth["mip"]) > allowed)[ok].any() or (np.abs(mn - truth["minip"]) > allowed)[ok].any()
    L = 8
    above = ok & (truth["mip"] > PJ_SR[0] + tol)
    rounded = (np.clip(np.round(truth["mip"] * L), 0, L - 1) + 0.5) / L
    assert (np.abs(rounded - truth["mip"]) > tol + 1.0 / (2 * L))[above].any()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["mip", "minip"])
def test_projection_device_meets_closed_form(proj_scene, mode):
    """GPU leg of pin 2, bound of test_projection_restatement_meets_closed_form: all four layouts, L = 1024 (render_proj_lds on
    the brick layouts) and 4096 (> TF_LDS_MAX: render_generic), range skipping on and off.  Jitter is not pinned here: it moves
    the ray within the +-1 pixel footprint as well as the start offset, which this per-ray bound does not cover.  L = 8 pins the
    TF bin rule."""
    sc = proj_scene
    truth, tol, hit = _proj_truth(sc)
    chord_vox = np.maximum(sc.far - sc.near, 0) * np.linalg.norm(sc.d * sc.ipw, axis=-1)
    margins = []
    for layout in sorted(LAYOUTS):
        for L in (8, 1024, 4096):
            r = _renderer(sc.grid, PJ_W, PJ_H, LAYOUTS[layout], _readback_tf(L), L)
            try:
                for skip in (False, True):
                    _set_params(r, sc.params(mode, L, dvr_skip_empty=skip, dvr_jitter=False))
                    r._check(r._lib.vx_render_frame(r._ctx, 0, 0.0))
                    margins.append(_check_projection(r.read_accum(), truth[mode], tol, chord_vox, L, hit))
            finally:
                r.close()
    print("projection margin", mode, max(margins))


# ==== 3. oblique slices and slabs against float64 resampling ==========================================================
SL_DIMS = (19, 27, 33)                  # z, y, x: ragged


def _slice_grid(oracle, spacing):
    rng = np.random.default_rng(23)
    vox = rng.integers(0, 3000, size=SL_DIMS, dtype=np.uint16)
    vox[9, 6:20, 10] = 4095                  # an L-shaped marker: a mirror or a transpose cannot map it onto itself
    vox[9, 6, 10:18] = 4095
    return oracle.BrickGrid(vox, spacing)


class SliceScene:
    def __init__(self, oracle, spacing):
        self.spacing = np.asarray(spacing, float)
        self.grid = _slice_grid(oracle, spacing)
        self.ext = tuple(int(e) for e in self.grid.index_extent)
        self.dec = CF.decode(oracle, self.grid)
        self.g = CF.neighbour_steps(self.dec)                 # zero padding included: planes leave the volume
        _, _, _, _, self.p = CF.make_pin_scene(self.grid, 64, 48, "dvr", (0.0, 0.0, -1.0), (0.0, 0.0, 0.0), (0, 0, 0),
                                               (1, 1, 1), (0.0, 0.0, -1.0), sample_range=(-1.0, 2.0))

    def centre(self, offset):
        if offset is None:
            return np.asarray(SL_FAR, float)
        data_mid = CF.index_to_world(np.array(SL_DIMS[::-1], float) / 2.0, self.ext, self.spacing)
        return data_mid + np.asarray(offset, float)

    def positions(self, center, normal, up, pixel, size, thickness, samples, mirror=False):
        """world positions (H, W, N, 3) of the plane, in float64: u = up_perp x n, v = up_perp, centred"""
        n = _normalised(normal)
        up = np.asarray(up, float)
        v = _normalised(up - np.dot(up, n) * n)
        u = np.cross(n, v) if mirror else np.cross(v, n)
        W, H = size
        x = (np.arange(W) - (W - 1) / 2) * pixel
        y = (np.arange(H) - (H - 1) / 2) * pixel
        s = (np.arange(samples) - (samples - 1) / 2) * (thickness / samples)
        return (np.asarray(center, float) + y[:, None, None, None] * v + x[None, :, None, None] * u
                + s[None, None, :, None] * n)

    def values(self, pos, shift=0.0):
        """float64 densities (H, W, N): zero-padded trilinear of the decoded voxels at the cell-frame position; density_scale *
        inv_maj = S * (1 / S) = 1 (S a power of two here)"""
        q = CF.world_to_index(pos, self.ext, self.spacing) - 0.5 + shift
        big = np.abs(q).max(axis=-1) > 2.0 ** 23
        v = CF.trilinear(self.dec, *[np.where(big, -8.0, q[..., a]) for a in range(3)])
        return v

    def bound(self, pos, reduce):
        """value error: fp32 positions -- each of origin, du, dv, dn rounded once (2^-24 relative) and three fma roundings of
        q, so per axis 4 * 2^-24 * (|origin| + (W-1)|du| + (H-1)|dv| + (N-1)|dn|), bounded by 4 * 2^-24 * 3 max|q| --
        times g_a; the trilinear's three mixes in fp32: 16 * 2^-24; the mean adds (N - 1) * 2^-24 * max|d| of the fp32 sum
        and 2^-24 of the division.  A plane whose every position lies more than 2 voxels (far more than the position error)
        outside the decoded volume on some axis reads 0 at every tap, before and after the +-2^24 clamp: its bound is 0, the
        value exactly 0"""
        q = CF.world_to_index(pos, self.ext, self.spacing) - 0.5
        dims = np.array(self.dec.shape[::-1])
        if (((q < -2.0) | (q > dims + 1.0)).any(axis=-1)).all():
            return 0.0
        qmax = np.abs(q).reshape(-1, 3).max(axis=0) + np.array(self.ext)
        b = float((12 * EPS32 * qmax * self.g).sum()) + 16 * EPS32
        if reduce == "mean":
            b += (pos.shape[2] - 1) * EPS32 * 1.0 + EPS32
        return b


SL_REDUCE = {"mean": lambda v: v.mean(axis=-1), "max": lambda v: v.max(axis=-1), "min": lambda v: v.min(axis=-1)}
SL_PLANE = dict(normal=(0.3, -0.5, 0.8), up=(0.1, 1.0, 0.2))
# (size, slab samples, thickness, centre, pixel size): partial waves and workgroups, planes partly outside the volume, one
# beyond the +-2^24 clamp.  The centre is a world offset from the data's centre (None: the absolute "far" centre).
SL_CASES = {"1x1": ((1, 1), 1, 0.0, (0.011, -0.007, 0.004), 0.01),
            "1x37": ((1, 37), 7, 0.05, (0.006, 0.003, -0.01), 0.009),
            "17x23_n4096": ((17, 23), 4096, 0.06, (0.01, -0.012, 0.004), 0.011),
            "300x257": ((300, 257), 7, 0.04, (0.01, -0.012, 0.004), 0.0021),
            "far": ((9, 7), 7, 0.1, None, 0.01)}
SL_FAR = (3.0e5, -2.0e5, 1.0e5)


def _slice_truth(sc, case, mirror=False, shift=0.0):
    size, N, th, c, px = SL_CASES[case]
    c = sc.centre(c)
    pos = sc.positions(c, SL_PLANE["normal"], SL_PLANE["up"], px, size, th, N, mirror=mirror)
    v = sc.values(pos, shift)
    return pos, {k: f(v) for k, f in SL_REDUCE.items()}


def _slice_plane(sc, obj, case):
    from volxel_amd import oblique
    size, N, th, c, px = SL_CASES[case]
    return oblique(obj, center=sc.centre(c), normal=SL_PLANE["normal"], up=SL_PLANE["up"], pixel_size=px, size=size, thickness=th,
                   samples=N)


@pytest.fixture(scope="module")
def slice_scenes():
    from oracle import oracle as O
    return {k: SliceScene(O, v) for k, v in SPACINGS.items()}


def test_slice_world_map_is_the_density_transform(slice_scenes):
    """the hand-derived world -> index map equals density_transform_inv of the uniforms in float64"""
    for sc in slice_scenes.values():
        m = np.asarray(sc.p.density_transform_inv[:], dtype=np.float64).reshape(4, 4).T
        w = np.array([[0.1, -0.2, 0.3], [0.0, 0.0, 0.0], [-0.4, 0.25, 0.05]])
        assert np.array_equal((m @ np.c_[w, np.ones(3)].T).T[:, :3], CF.world_to_index(w, sc.ext, sc.spacing))


@pytest.mark.parametrize("case", sorted(SL_CASES))
@pytest.mark.parametrize("spacing", sorted(SPACINGS))
def test_slice_restatement_meets_closed_form(slice_scenes, spacing, case):
    """CPU leg of pin 3: slice_ref.values of mpr.oblique's plane against the float64 resampling (SliceScene.bound derives the
    tolerance); the plane partly leaves the volume (taps read 0) and "far" lies beyond the +-2^24 clamp (all 0)"""
    from types import SimpleNamespace
    from tests import slice_ref as SR
    sc = slice_scenes[spacing]
    pos, truth = _slice_truth(sc, case)
    sp = _slice_plane(sc, SimpleNamespace(_params=sc.p), case)
    for reduce, want in truth.items():
        got = SR.values(sp, sc.grid, sc.p, reduce=SR.REDUCE_IDS[reduce])
        b = sc.bound(pos, reduce)
        assert float(np.abs(got - want).max()) <= b, (reduce, float(np.abs(got - want).max()), b)
        if case == "far":
            assert b == 0.0 and (got == 0).all() and (want == 0).all()
    if case != "far":
        assert float(truth["max"].max()) > 0.1
    if case == "300x257":
        assert (truth["max"] == 0).any()          # part of the plane lies outside the volume


def test_slice_negative_controls(slice_scenes):
    """outside the same tolerance: the plane mirrored (+x = normal x up), transposed (u and v swapped), and the positions
    shifted by half a voxel (cell frame = index position instead of index - 1/2)"""
    sc = slice_scenes["aniso"]
    pos, truth = _slice_truth(sc, "300x257")
    b = sc.bound(pos, "max")
    _, mir = _slice_truth(sc, "300x257", mirror=True)
    assert float(np.abs(mir["max"] - truth["max"]).max()) > 100 * b
    _, sh = _slice_truth(sc, "300x257", shift=0.5)
    assert float(np.abs(sh["max"] - truth["max"]).max()) > 100 * b
    size, N, th, c, px = SL_CASES["17x23_n4096"]
    p2 = sc.positions(sc.centre(c), SL_PLANE["normal"], SL_PLANE["up"], px, (17, 17), th, 1)
    tr = np.swapaxes(p2, 0, 1)
    assert float(np.abs(sc.values(tr) - sc.values(p2)).max()) > 100 * sc.bound(p2, "mean")


def _display_checks(vals_ref, rgba_grey, rgba_tf, b, window):
    """bytes within one code of the float64 value: grey c = (v - w0) / (w1 - w0) clamped, |byte - 255 c| <= 1/2 + 255 (b /
    (w1 - w0) + 4 * 2^-24); TF r = g = b = (i + 1/2) / L, L = 1024: the bin centre is within 1 / (2L) + b of v, |byte - 255 v| <=
    1/2 + 255 / 2048 + 255 (b + 4 * 2^-24)"""
    w0, w1 = window
    c = np.clip((vals_ref - w0) / (w1 - w0), 0.0, 1.0) * 255.0
    e = np.abs(rgba_grey[..., :3].astype(np.float64) - c[..., None])
    assert float(e.max()) <= 0.5 + 255.0 * (b / (w1 - w0) + 4 * EPS32) <= 1.0, float(e.max())
    e = np.abs(rgba_tf[..., :3].astype(np.float64) - 255.0 * np.clip(vals_ref, 0.0, 1.0)[..., None])
    assert float(e.max()) <= 0.5 + 255.0 / 2048 + 255.0 * (b + 4 * EPS32) <= 1.0, float(e.max())
    assert (rgba_grey[..., 3] == 255).all() and (rgba_tf[..., 3] == 255).all()


def test_slice_display_restatement_bytes(slice_scenes):
    from types import SimpleNamespace
    from tests import slice_ref as SR
    sc = slice_scenes["iso"]
    pos, truth = _slice_truth(sc, "300x257")
    sp = _slice_plane(sc, SimpleNamespace(_params=sc.p), "300x257")
    vals = SR.values(sp, sc.grid, sc.p, reduce=SR.MAX)
    q = type(sp).from_buffer_copy(sp)
    q.window[0], q.window[1] = 0.1, 0.9
    grey = SR.display(vals, q, mode=SR.GREY)
    tf = SR.display(vals, q, _readback_tf(1024), 1024, (-1.0, 2.0), mode=SR.TF)
    _display_checks(truth["max"], grey, tf, sc.bound(pos, "max"), (0.1, 0.9))


@pytest.mark.gpu
@pytest.mark.parametrize("spacing", sorted(SPACINGS))
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_slice_device_meets_closed_form(slice_scenes, layout, spacing):
    """GPU leg of pin 3: vx_slice of every case and reduction against the float64 resampling with SliceScene.bound; the grey
    and TF displays of the 300 x 257 max slab as bytes within one code (bricku8 slices the reference textures)"""
    sc = slice_scenes[spacing]
    r = _renderer(sc.grid, 64, 48, LAYOUTS[layout], _readback_tf(1024), 1024)
    worst = 0.0
    try:
        r.settings.sample_range = (-1.0, 2.0)
        r.settings.render_mode = "dvr"
        r.bind_uniforms()
        for case in sorted(SL_CASES):
            pos, truth = _slice_truth(sc, case)
            sp = _slice_plane(sc, r, case)
            for reduce, want in truth.items():
                b = sc.bound(pos, reduce)
                if case == "300x257" and reduce == "max":
                    vals, grey = r.slice(sp, reduce=reduce, display="grey", window=(0.1, 0.9))
                    _, tf = r.slice(sp, reduce=reduce, display="tf")
                    _display_checks(want, grey, tf, b, (0.1, 0.9))
                else:
                    vals = r.slice(sp, reduce=reduce)
                err = float(np.abs(vals - want).max())
                assert err <= b, (case, reduce, err, b)
                if case == "far":
                    assert b == 0.0 and (vals == 0).all()      # beyond the +-2^24 clamp: exactly 0
                else:
                    worst = max(worst, err / b)
    finally:
        r.close()
    print("slice margin", layout, spacing, worst)
