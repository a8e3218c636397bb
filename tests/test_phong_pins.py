"""Closed-form pins for Phong-shaded DVR (dvr_phong).

The C oracle, its NumPy twin and the kernels were written together; they agree with each other to 1e-5, so an error they
share passes every parity test.  Here the `dvr_phong` image is held to answers computed in float64 from the scene alone
(tests/closed_form.py: spacing and extent, camera position / look-at / fov, the clip box, the light, the TF entries, the
Phong constants) on three fields built as u16 stacks:

  1. a flat field: the gradient is exactly 0, Phong leaves the TF colour alone -- `dvr_phong` equals `dvr` bit for bit;
  2. a linear ramp along a world direction m off every axis: the normal is the constant -m, a constant-alpha TF cut by
     sample_range at an iso-plane gives (1 - T_end) (c (ka + kd max(0, n.l)) + ks max(0, n.h)^s) K per pixel;
  3. an ellipsoidal bowl f = A - B |w - c|^2, isotropic in world space: the central difference of the trilinear of a separable
     quadratic is exactly twice its derivative, so the normal at every sample is (w - c) / |w - c|; sample_range cuts a lit ball.

Two tiers per field, as the shadow pin has.  Tier 1 (analytic) uses the field's exact densities and normals and bounds what
the brick codec may move (its voxel error eps, measured with decode()).  Tier 2 (contract) evaluates the march contract and the
Phong rule in float64 on the decoded voxels and bounds only fp32 and the hardware rsq / log2 / exp2.  Every pin has a CPU leg
(the oracle) and a GPU leg (`gpu`: layouts 0, 1, 2 and 4, exact empty-space skipping on and off), and a set of deliberately
wrong float64 models that must break the tier-2 bound of their case (test_phong_negative_controls)."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import closed_form as CF
from tests import common
from tests.shapes import DIMS, FIELD_RES, SPACINGS, Case, Field, field_params, field_rays, true_grad

EPS32 = 2.0 ** -24
LAYOUTS = {k: common.LAYOUTS[k] for k in ("reference", "cellquad", "brickf32", "bricku8")}
W, H = FIELD_RES
COLOUR = np.array([0.8, 0.5, 0.3])


def _cases(fields):
    F = fields
    L_OBL = (-0.4, -0.75, 0.53)
    return {
        "flat_iso": Case(F["flat", "iso"], (0.3, 0.25, -0.6), L_OBL, (0.3, 0.7, 0.4, 32.0)),
        "flat_aniso_ortho": Case(F["flat", "aniso"], (0.3, 0.25, -0.6), L_OBL, (0.3, 0.7, 0.4, 32.0), ortho=0.3),
        "ramp_iso_default": Case(F["ramp", "iso"], (0.3, 0.25, -0.6), L_OBL, (0.3, 0.7, 0.4, 32.0)),
        "ramp_aniso_ortho_ka": Case(F["ramp", "aniso"], (-0.2, 0.3, -0.6), L_OBL, (1.0, 0.0, 0.0, 8.0), step=0.125, ortho=0.25),
        "ramp_aniso_kd_step3": Case(F["ramp", "aniso"], (0.35, -0.2, -0.55), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0, 1.0), step=3.0),
        "ramp_iso_inside_ks64": Case(F["ramp", "iso"], (0.02, 0.01, -0.03), L_OBL, (0.0, 0.0, 1.0, 64.0),
                                     look_off=(0.3, -0.2, 0.5), inside=True),
        "ramp_aniso_s0_maxsteps": Case(F["ramp", "aniso"], (0.3, 0.25, -0.6), (-0.7, 0.2, 0.68), (0.0, 0.0, 1.0, 0.0), max_steps=12),
        "bowl_iso_default": Case(F["bowl", "iso"], (0.3, 0.25, -0.6), L_OBL, (0.3, 0.7, 0.4, 32.0)),
        "bowl_aniso_ortho_ks64": Case(F["bowl", "aniso"], (-0.25, 0.3, -0.6), L_OBL, (0.0, 0.0, 1.0, 64.0), step=0.125, ortho=0.12),
        "bowl_aniso_axis_kd": Case(F["bowl", "aniso"], (0.3, 0.25, -0.6), (0.0, -1.0, 0.0), (0.0, 1.0, 0.0, 8.0)),
        "bowl_iso_persp_ks8": Case(F["bowl", "iso"], (0.5, 0.1, -0.4), (-0.6, -0.2, 0.77), (0.0, 0.0, 1.0, 8.0)),
        # shininess 0 with ks alone: the spec is ks at every shaded sample, on the back-facing half (n.h <= 0) too
        "bowl_aniso_s0": Case(F["bowl", "aniso"], (-0.3, -0.25, -0.6), L_OBL, (0.0, 0.0, 1.0, 0.0)),
        "bowl_aniso_ka_step3": Case(F["bowl", "aniso"], (0.3, 0.25, -0.6), L_OBL, (1.0, 0.0, 0.0, 1.0), step=3.0, ortho=0.12),
        # the camera looks toward the light: the directional background's highlight (d.l)^300 lies on the image
        "bowl_iso_ert_env": Case(F["bowl", "iso"], (0.25, 0.2, -0.6), None, (0.3, 0.7, 0.4, 8.0), alpha=0.6,
                                 ert_eps=0.05, env=True),
    }


def _gain(env):
    """K = albedo mis f_p Le (fragment.frag:94-97): mis = 1 / (1 + f_p^2) with the environment shown, else 1"""
    f_p = 1.0 / (4.0 * math.pi)
    return 0.9 * (1.0 / (1.0 + f_p * f_p) if env else 1.0) * f_p * 4.01


class Model:
    """the dvr_phong image of a case in float64 (tier 2 unless `analytic`), with its per-pixel tolerance and sample counts.

    Variants (negative controls): flip (normal +g/|g|), aniso_inverted (gradient times spacing instead of divided),
    half_taps (taps at q +- 1/2), light_flipped, half_plus_d (h from +ray.d), reflect (Phong's r = 2 (n.l) n - l with v in
    place of n and h), swap_ka_kd, spec_tinted, shininess_ignored (s = 1), ert_keeps_T (the background behind rays ERT ended)."""

    def __init__(self, case, analytic=False, variant=None):
        fd, self.case = case.field, case
        o, d = field_rays(case)
        self.d = d
        lo, hi = CF.world_box(fd.ext, fd.spacing, *fd.clip())
        dt, x, n, valid, pos = CF.march_samples(o, d, lo, hi, fd.ipw, case.step, case.max_steps)
        q = CF.world_to_index(pos, fd.ext, fd.spacing) - 0.5
        ka, kd, ks, shin = case.phong
        light = -case.light if variant == "light_flipped" else case.light
        if variant == "swap_ka_kd":
            ka, kd = kd, ka
        if variant == "shininess_ignored":
            shin = 1.0
        S = CF.world_scale(fd.ext, fd.spacing)
        sigma = case.alpha * S                                  # alpha volume_maj per world unit, volume_maj = S
        if analytic:
            dens = fd.f(pos) if fd.kind != "flat" else np.full(q.shape[:-1], 0.5)
            nrm = fd.normal(pos) if fd.kind != "flat" else np.zeros(q.shape)
            shaded = np.linalg.norm(nrm, axis=-1) > 0
            gmag = np.ones(q.shape[:-1])
        else:
            if variant == "half_taps":
                dens = CF.trilinear(fd.dec, *np.moveaxis(q, -1, 0))
                D = np.stack([CF.trilinear(fd.dec, *np.moveaxis(q + 0.5 * e, -1, 0)) -
                              CF.trilinear(fd.dec, *np.moveaxis(q - 0.5 * e, -1, 0)) for e in np.eye(3)], axis=-1)
            else:
                dens, D = CF.central_differences(fd.dec, q)
            G = D * (fd.spacing if variant == "aniso_inverted" else fd.ipw)       # world gradient / density_scale
            gmag = np.linalg.norm(G, axis=-1)
            shaded = (S * gmag) ** 2 > 1e-12                    # the g2 > 1e-12 branch on g = density_scale G
            nrm = np.where(shaded[..., None], -G / np.where(shaded, gmag, 1.0)[..., None], 0.0)
        if variant == "flip":
            nrm = -nrm
        dd = d[..., None, :]
        h = CF.half_vector(light, -dd if variant == "half_plus_d" else dd)
        col = np.broadcast_to(COLOUR, q.shape)
        if variant == "reflect":
            l = -light
            r = 2.0 * (nrm * l).sum(axis=-1, keepdims=True) * nrm - l
            rgb = CF.blinn_phong(col, nrm, light, np.ones(1), ka, kd, 0.0, 1.0) + ks * (
                np.maximum(0.0, (r * -dd).sum(axis=-1)) ** shin)[..., None]
        else:
            rgb = CF.blinn_phong(col, nrm, light, h, ka, kd, ks, shin)
            if variant == "spec_tinted":
                base = CF.blinn_phong(col, nrm, light, h, ka, kd, 0.0, shin)
                rgb = base + col * (rgb - base)
        rgb = np.where(shaded[..., None], rgb, col)
        inr = valid & (dens >= fd.cut) & (dens <= 1.0)
        tau = np.cumsum(np.where(inr, sigma * dt[..., None], 0.0), axis=-1)
        ert = -math.log(case.ert_eps)
        fired = inr & (tau >= ert)
        first = np.where(fired.any(axis=-1), fired.argmax(axis=-1), valid.shape[-1])
        live = np.arange(valid.shape[-1]) <= first[..., None]
        used = inr & live
        T_prev = np.exp(-np.concatenate([np.zeros(tau.shape[:-1] + (1,)), tau[..., :-1]], axis=-1))
        dT = np.where(used, T_prev - np.exp(-tau), 0.0)
        self.K = _gain(case.env)
        img = self.K * (dT[..., None] * rgb).sum(axis=-2)
        terminated = fired.any(axis=-1)
        T_end = np.where(terminated, 0.0, np.exp(-np.where(inr, sigma * dt[..., None], 0.0).sum(axis=-1)))
        if variant == "ert_keeps_T":
            T_end = np.exp(-np.where(used, sigma * dt[..., None], 0.0).sum(axis=-1))
        if case.env:
            img = img + T_end[..., None] * CF.directional_environment(d, light)[..., None]
        self.img, self.T_end, self.terminated = img, T_end, terminated
        self.capped = (n >= case.max_steps) & (x > case.max_steps)
        self.back_facing = (used & ((nrm * h).sum(axis=-1) < 0)).any()
        self.eye_inside = bool(((case.eye >= lo) & (case.eye <= hi)).all())
        self.samples = (valid & live).sum(axis=-1)
        self.grads = used.sum(axis=-1)
        self.smax = float(np.abs(rgb).max()) if rgb.size else 1.0
        self.sigma_dt = sigma * dt
        self._tolerance(fd, case, analytic, q, dens, nrm, gmag, shaded, inr, valid, tau, ert, x, n, dT, light, h)

    def _tolerance(self, fd, case, analytic, q, dens, nrm, gmag, shaded, inr, valid, tau, ert, x, n, dT, light, h):
        _, kd, ks, shin = case.phong
        # sample positions: fp32 ray set-up and q = fma(k, dq, q0) -- four ulps of the largest quantity a position is formed
        # from (|q| and the ray's length in voxels)
        qabs = float(np.abs(np.where(valid[..., None], q, 0.0)).max()) + 64.0
        dq = 4.0 * 2.0 ** -23 * qabs
        g = CF.neighbour_steps(fd.dec)                       # Lipschitz of the trilinear per axis
        if analytic:
            # the codec moves every voxel by <= eps: each of T(c + e_i), T(c - e_i) by eps, D_i by 2 eps, the world gradient
            # 2 G_true by 2 eps ipw_i per axis; the trilinear of the field adds its curvature term to the density
            eps = fd.eps()
            err_G = 2.0 * eps * np.linalg.norm(fd.ipw) * np.ones(q.shape[:-1])
            dn = np.minimum(2.0, 2.0 * err_G / np.maximum(true_grad(fd, q), 1e-300))
            d_band = eps + fd.curvature() + float(g.sum()) * dq + 4 * EPS32
        else:
            # fp32: each trilinear within 8 ulps of 1, D_i within 2^-20; a position error dq moves D_i by at most
            # sum_j |dD_i/dq_j| dq, |dD_i/dq_j| <= max |D_j dec(x) - D_j dec(x - 2 e_i)| (a convex combination of those)
            M = np.zeros((3, 3))
            for i in range(3):
                for j in range(3):
                    Dj = np.diff(fd.dec, axis=2 - j)
                    sh = [slice(None)] * 3
                    sh2 = [slice(None)] * 3
                    sh[2 - i], sh2[2 - i] = slice(2, None), slice(None, -2)
                    M[i, j] = float(np.abs(Dj[tuple(sh)] - Dj[tuple(sh2)]).max())
            dD = 2.0 ** -20 + M.sum(axis=1) * dq
            err_G = np.linalg.norm(dD * fd.ipw) * np.ones(q.shape[:-1])
            dn = np.minimum(2.0, 2.0 * err_G / np.maximum(gmag, 1e-300))
            # within fp32 of the range threshold: the density's rounding and its position error
            d_band = 2.0 ** -20 + float(g.sum()) * dq
        ndh = np.maximum(0.0, (nrm * h).sum(axis=-1))
        lip_spec = ks * shin * np.minimum(1.0, ndh + dn) ** max(shin - 1.0, 0.0) if shin >= 1 else 0.0 * ndh
        e_shade = np.where(shaded, float(COLOUR.max()) * kd * dn + lip_spec * dn, 0.0) + 4e-6 * (1 + ks)
        amb_range = valid & (np.abs(dens - fd.cut) <= d_band)
        # tau within rounding of the ERT threshold, or within the optical depth of the range decisions before it that may
        # go either way
        band = 1e-5 * ert + np.cumsum(amb_range, axis=-1) * self.sigma_dt[..., None]
        amb_ert = (inr | amb_range) & (np.abs(tau - ert) <= band)
        amb_count = (np.abs(x - np.round(x)) < 2e-3) & (n < case.max_steps)
        env = CF.directional_environment(self.d, light) if case.env else 0.0 * n
        # one sample counted or not: its own dT (<= (1 - exp(-sigma dt))) and every later dT and T_end scaled by
        # exp(+-sigma dt): at most (exp(sigma dt) - 1) (2 K smax + background)
        one = np.expm1(self.sigma_dt) * (2.0 * self.K * max(self.smax, 1.0) + env)
        n_amb = amb_range.sum(axis=-1) + amb_count
        tol = self.K * ((dT * e_shade).sum(axis=-1) + 3e-5 * (self.smax + 1.0) + n * EPS32 * self.smax) + n_amb * one
        # ERT on a sample within rounding of the threshold: the ray's T_end is 0 or exp(-ert) = epsilon, and its colour
        # moves by at most epsilon times the largest shade
        tol = tol + amb_ert.any(axis=-1) * (case.ert_eps * (env + self.K * self.smax)) + env * 1e-5
        if case.env:
            # the background's c = max(0, d.l) in fp32 from the device's own ray: within 2^-20; 4 c^300 moves by 1200 c^299 that
            c = np.clip((self.d * -light).sum(axis=-1) + 2.0 ** -20, 0.0, 1.0)
            tol = tol + self.T_end * 1200.0 * c ** 299 * 2.0 ** -20 + 4 * EPS32 * env
        self.tol = tol
        self.exact_count = ~(amb_count | amb_range.any(axis=-1) | amb_ert.any(axis=-1))
        # a ray with an ambiguous decision may take one sample more than the float64 march and, where ERT is in doubt, shade
        # every sample it has: its count may differ by up to n + 1
        self.count_slack = int((n + 1)[~self.exact_count].sum())

    def check(self, img):
        """per pixel and channel |img - model| <= tol; returns observed / allowed"""
        err = np.abs(img[..., :3].astype(np.float64) - self.img)
        ok = err <= self.tol[..., None]
        assert ok.all(), (int((~ok).sum()), float((err / self.tol[..., None]).max()))
        return float((err / self.tol[..., None]).max())


def _case_tf(case, L=16):
    """every entry the colour and the case's alpha: the NEAREST bin cannot matter, only sample_range does"""
    return np.tile(np.array([*COLOUR, case.alpha], dtype=np.float32), (L, 1)).reshape(-1)


@pytest.fixture(scope="module")
def fields():
    from oracle import oracle as O
    return {(k, sp): Field(O, k, SPACINGS[sp]) for k in ("flat", "ramp", "bowl") for sp in SPACINGS}


@pytest.fixture(scope="module")
def cases(fields):
    return _cases(fields)


@pytest.fixture(scope="module")
def models(cases):
    return {name: Model(c) for name, c in cases.items()}


CASES = ["flat_iso", "flat_aniso_ortho", "ramp_iso_default", "ramp_aniso_ortho_ka", "ramp_aniso_kd_step3",
         "ramp_iso_inside_ks64", "ramp_aniso_s0_maxsteps", "bowl_iso_default", "bowl_aniso_ortho_ks64", "bowl_aniso_axis_kd",
         "bowl_iso_persp_ks8", "bowl_aniso_s0", "bowl_aniso_ka_step3", "bowl_iso_ert_env"]
FIELD_CASES = [c for c in CASES if not c.startswith("flat")]


def test_phong_scene_geometry_is_hand_derived(fields):
    """the hand-written maps equal the uniforms: density_transform_inv's diagonal is index per world (S / spacing),
    volume_maj = volume_density_scale = S, and the clip box, camera and light reach the uniforms as given"""
    for (kind, sp), fd in fields.items():
        p = field_params(Case(fd, (0.3, 0.25, -0.6), (0.0, -1.0, 0.0), (0.3, 0.7, 0.4, 32.0)), "dvr_phong")
        m = np.asarray(p.density_transform_inv[:], dtype=np.float64).reshape(4, 4).T
        assert np.allclose(np.diag(m)[:3], fd.ipw, rtol=1e-7, atol=0)
        S = CF.world_scale(fd.ext, fd.spacing)
        assert p.volume_maj == np.float32(S) and p.volume_density_scale == np.float32(S)
        lo, hi = CF.world_box(fd.ext, fd.spacing, *fd.clip())
        assert np.allclose(p.volume_aabb_min[:], lo, atol=1e-7) and np.allclose(p.volume_aabb_max[:], hi, atol=1e-7)


def test_phong_fields_are_what_they_claim(fields):
    """the flat field decodes to exactly 1/2 wherever its taps reach; the ramp's and the bowl's codec error is small next to
    their central differences, and the bowl's trilinear central difference is exactly twice its derivative"""
    for sp in SPACINGS:
        fd = fields["flat", sp]
        (lo, hi) = fd.clip()
        a = np.floor(np.array(lo) * 64 - 2).astype(int)
        b = np.ceil(np.array(hi) * 64 + 2).astype(int)
        assert (fd.dec[a[2]:b[2], a[1]:b[1], a[0]:b[0]] == 0.5).all()
        for kind in ("ramp", "bowl"):
            fd = fields[kind, sp]
            assert fd.eps() < 2e-3, (kind, sp, fd.eps())
    # exactness of the central difference on the float64 field itself (no codec): the ideal voxels of the bowl
    fd = fields["bowl", "aniso"]
    ideal = np.zeros_like(fd.dec)
    nz, ny, nx = DIMS
    ideal[:nz, :ny, :nx] = fd.ideal
    rng = np.random.default_rng(3)
    q = rng.uniform([2, 2, 2], [nx - 4, ny - 4, nz - 4], size=(200, 3))      # every tap inside the data
    _, D = CF.central_differences(ideal, q)
    w = CF.index_to_world(q + 0.5, fd.ext, fd.spacing)
    grad_idx = -2.0 * fd.B * (w - fd.c) / fd.ipw            # df/dindex_i = df/dw_i dw_i/dindex_i
    assert np.abs(D - 2.0 * grad_idx).max() <= 1e-12


def _tier1_check(case, img):
    """tier 1: |img - analytic model| <= analytic tolerance (the codec's eps through the gradient, the normal and the range)"""
    m = Model(case, analytic=True)
    return m.check(img)


@pytest.mark.parametrize("name", CASES)
def test_phong_oracle_meets_closed_form(cases, models, name):
    """CPU leg: the oracle's dvr_phong image against the float64 models of Model, both tiers, and its counters against the
    float64 march.

    Tier 2 (contract), per pixel and channel, in units of K:
      * shading: per contributing sample dT_k e_k, e_k = (c kd + ks s min(1, n.h + dn)^(s-1)) dn (the Lipschitz constants of
        the diffuse and specular terms in n; s = 0: no term) + 4e-6 (1 + ks) for rsq / log2 / exp2 (1 ulp each: the pow error
        is below 2^-23 (1 + s |log2 x| x^s) <= 2^-22); dn = 2 |dG| / |G| bounds the normal's error from a gradient error dG:
        dD_i = 2^-20 (two fp32 trilinears, 8 ulp each) + sum_j M_ij dq, M_ij = max |D_j dec(x) - D_j dec(x - 2 e_i)| the
        largest change of D_i per voxel along j, dq four ulps of the largest position magnitude (fp32 ray set-up and fma walk);
      * compositing: 3e-5 (smax + 1) for exp and the colour fma chain (as the goldens' 1e-5 Phong tolerance, widened for the
        brightest shade), n 2^-24 smax for the n roundings of tau;
      * a sample whose density lies within 2^-20 + sum_a g_a dq of the cut (g_a the trilinear's Lipschitz per axis) or a ray
        whose (far - t0) / dt lies within 2e-3 of an integer may go either way in fp32: each such sample moves the pixel by at
        most its own dT and the change of all later dT and of T_end, (exp(sigma dt) - 1) (2 K max(smax, 1) + background);
      * ERT within 1e-5 of its threshold: epsilon times (the background + K smax); the background itself: 4 2^-24 relative
        and 1200 c^299 2^-20 for its c^300 term.
    Tier 1 (analytic) replaces the decoded voxels by the field: the gradient's error per axis is 2 eps ipw_i, the range band
    eps + sum_a a_a / 4 (the trilinear's error on the bowl's quadratic; 0 on the ramp).
    Counters: samples per ray and grad_samples exactly, except on the rays with an ambiguous decision above."""
    from oracle import oracle as O
    c, m = cases[name], models[name]
    p = field_params(c, "dvr_phong")
    img, oc, per_ray = O.render(p, c.field.grid, _case_tf(c), 16, ray_samples=True)
    margin = m.check(img)
    assert float(m.img.max()) > 0.02, "the case shows nothing"
    # each case exercises what its name says
    assert m.eye_inside == c.inside
    assert m.capped.any() == (c.max_steps < 1 << 20)
    if c.env:
        assert m.terminated.sum() >= 10 and (~m.terminated & (m.grads > 0)).sum() >= 10
    if c.phong[3] == 0 and c.field.kind == "bowl":
        assert m.back_facing
    ex = m.exact_count
    assert ex.sum() >= 0.9 * ex.size
    assert np.array_equal(per_ray[ex], m.samples[ex])
    assert abs(int(oc.grad_samples) - int(m.grads.sum())) <= m.count_slack
    assert oc.grad_samples == oc.tf_samples                      # constant alpha > 0: every in-range sample is shaded
    t1 = _tier1_check(c, img)
    print(name, "tier 2 margin", margin, "tier 1 margin", t1)


@pytest.mark.parametrize("spacing", sorted(SPACINGS))
def test_phong_flat_field_equals_dvr_on_the_oracle(fields, spacing):
    """pin 1, CPU leg: on the flat field every gradient is exactly 0, so the g2 > 1e-12 branch leaves the TF colour unshaded
    and dvr_phong composites exactly what dvr does: the images are equal bit for bit, and every sample is a gradient sample"""
    from oracle import oracle as O
    for name in ("flat_iso", "flat_aniso_ortho"):
        c = _cases(fields)[name]
        if c.field is not fields["flat", spacing]:
            continue
        a, ca = O.render(field_params(c, "dvr"), c.field.grid, _case_tf(c), 16)
        b, cb = O.render(field_params(c, "dvr_phong"), c.field.grid, _case_tf(c), 16)
        assert np.array_equal(a, b)
        assert cb.grad_samples == cb.samples == ca.samples > 100


def test_phong_negative_controls(cases, models):
    """each wrong float64 model breaks the tier-2 bound of its case on some pixel by more than twice the tolerance (the device
    and the oracle lie within one tolerance of the right model, so a kernel that made the error would fail):
      the normal flipped (+g/|g|), the anisotropic map inverted (D times spacing), taps at q +- 1/2, the light's sign flipped,
      h from +ray.d, Phong's reflection vector for Blinn's h, ka and kd swapped, the spec tinted by the TF colour, the
      shininess ignored, and T kept at ERT (the background behind the rays ERT ended).  Measured: 25x to 1800x the bound,
      except the +-1/2 taps (about 2.5x): on a smooth field they change the gradient's length far more than its direction."""
    controls = {"flip": "bowl_iso_default", "aniso_inverted": "bowl_aniso_axis_kd", "half_taps": "bowl_iso_persp_ks8",
                "light_flipped": "ramp_aniso_kd_step3", "half_plus_d": "bowl_iso_persp_ks8", "reflect": "bowl_iso_persp_ks8",
                "swap_ka_kd": "bowl_iso_default", "spec_tinted": "bowl_iso_persp_ks8", "shininess_ignored": "bowl_iso_persp_ks8",
                "ert_keeps_T": "bowl_iso_ert_env"}
    for variant, name in controls.items():
        m = models[name]
        wrong = Model(cases[name], variant=variant)
        gap = np.abs(wrong.img - m.img) / (2.0 * m.tol[..., None])
        assert float(gap.max()) > 1.0, (variant, name, float(gap.max()))
    # the flipped normal breaks the loose tier-1 bound too
    m1 = Model(cases["bowl_iso_default"], analytic=True)
    wrong = Model(cases["bowl_iso_default"], variant="flip")
    assert float((np.abs(wrong.img - m1.img) / (2.0 * m1.tol[..., None])).max()) > 1.0


def _render(case, mode, layout, skip):
    from volxel_amd import Volxel3DRenderer
    fd = case.field
    r = Volxel3DRenderer(W, H, layout=LAYOUTS[layout])
    try:
        r.setup_from_grid(fd.grid)
        r.change_transfer_func(_case_tf(case), 16)
        r._check(r._lib.vx_set_params(r._ctx, C.byref(field_params(case, mode, skip))))
        r.reset_counters()
        r._check(r._lib.vx_render_frame(r._ctx, 0, 0.0))
        return r.read_accum(), r.counters()
    finally:
        r.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", CASES)
def test_phong_device_meets_closed_form(cases, models, name):
    """GPU leg: every layout (the LDS-window Phong kernel on brickf32 / bricku8, the generic kernel on reference / cellquad),
    exact empty-space skipping off and on, against the tier-2 and tier-1 bounds of test_phong_oracle_meets_closed_form; the
    counters: samples (skipping off) and grad_samples exactly against the float64 march, except for rays with an ambiguous
    decision.  On the flat field the dvr_phong image equals the dvr image bit for bit and grad_samples == samples."""
    c, m = cases[name], models[name]
    ex = m.exact_count
    margins = []
    for layout in sorted(LAYOUTS):
        for skip in (False, True):
            img, cnt = _render(c, "dvr_phong", layout, skip)
            margins.append(m.check(img))
            _tier1_check(c, img)
            slack = m.count_slack
            assert abs(int(cnt.grad_samples) - int(m.grads.sum())) <= slack, (layout, skip, cnt.grad_samples, m.grads.sum())
            if not skip:
                assert abs(int(cnt.samples) - int(m.samples.sum())) <= slack, (layout, cnt.samples, m.samples.sum())
                if ex.all():
                    assert cnt.samples == int(m.samples.sum())
            if name.startswith("flat"):
                dvr, cd = _render(c, "dvr", layout, skip)
                assert np.array_equal(dvr, img), (layout, skip)
                assert cnt.grad_samples == cnt.samples == cd.samples, (layout, skip)
    print(name, "device tier-2 margin", max(margins))
