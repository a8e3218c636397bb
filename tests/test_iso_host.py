"""Isosurfaces without a GPU (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): the ABI of VxIsoParams and the entry points, the
refusals, the Node host carrying the new calls, and the NumPy restatement (tests/iso_ref.py) held to float64 closed forms.

The pins use the ramp, bowl and flat fields of tests/test_phong_pins.py in two tiers, as the Phong pins do:
  * tier 2 (contract): the march, the first-hit rule and the bisection evaluated in float64 on the decoded voxels.  Every decision
    whose float64 density lies outside the fp32 band of the threshold is taken alike, so on those rays the hit flag, k and s*
    must be EQUAL and t, w within the rounding of the fp32 ray set-up; the normal within the bound a gradient error gives it;
  * tier 1 (analytic): the field itself.  The ramp's hit lies on its iso-plane and the bowl's on the sphere of radius
    sqrt((A - iso) / B), within dt 2^-refine (the last bracket) plus the codec's density error over the field's slope along the
    ray; the normal is -m on the ramp and radial on the bowl.
Deliberately wrong float64 models (the hit at sample k unrefined, s* = lo, a half-sample offset either way, a flipped normal, a
cap shaded with the field's gradient) must break the tier-2 bound of their case."""
import ctypes as C
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import closed_form as CF
from tests import iso_ref as IR
from tests.common import F32, NAPI, ROOT
from tests.shapes import ISO_CASES as CASES
from tests.shapes import ISO_COLOUR as COLOUR
from tests.shapes import ISO_PHONG as PHONG
from tests.shapes import RAMP_M, SPACINGS, Field, field_rays, iso_params, phong_case, true_grad

EPS32 = 2.0 ** -24


# ---- the boundary ------------------------------------------------------------------------------------------------------
def test_iso_params_layout_matches_the_c_compiler(tmp_path):
    from volxel_amd import _abi, VxIsoParams
    assert VxIsoParams is _abi.VxIsoParams
    names = [f[0] for f in VxIsoParams._fields_]
    assert names == ["iso", "color", "ka", "kd", "ks", "shininess", "refine", "skip", "window"]
    src = tmp_path / "iso.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "volxel_hip.h"\n'
                   'int main(void) { printf("%u' + " %u" * len(names) + '\\n", (unsigned)sizeof(VxIsoParams)'
                   + "".join(", (unsigned)offsetof(VxIsoParams, %s)" % n for n in names) + "); return 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "iso")])
    got = [int(x) for x in subprocess.check_output([str(tmp_path / "iso")]).split()]
    assert got == [C.sizeof(VxIsoParams)] + [getattr(VxIsoParams, n).offset for n in names]
    assert got[0] == 4 * (1 + 3 + 4 + 1 + 1 + 4)


def test_iso_entry_points_are_declared_and_exported(native_lib):
    from volxel_amd import _abi
    for name in ("vx_isosurface", "vx_iso_stats"):
        assert name in _abi.declared_symbols("volxel_hip.h")
        getattr(native_lib, name)


def test_c_refusals_without_a_context(native_lib):
    from volxel_amd import _abi
    q = _abi.VxIsoParams()
    invalid = _invalid_code()
    assert native_lib.vx_isosurface(None, C.byref(q), None, None) == invalid
    assert native_lib.vx_isosurface(None, None, None, None) == invalid
    assert native_lib.vx_iso_stats(None, None, None, None, None, None, None) == invalid


def _invalid_code():
    import re
    text = open(os.path.join(ROOT, "include", "volxel_hip.h")).read()
    return int(re.search(r"#define VX_ERR_INVALID (\d+)", text).group(1))


def test_python_refusals():
    import types
    from volxel_amd import Volxel3DRenderer
    r = object.__new__(Volxel3DRenderer)      # the checks come before any library call
    r._ctx = None
    r.width, r.height = 32, 24
    r.settings = types.SimpleNamespace(phong=PHONG)
    bad = [dict(iso=float("nan")), dict(iso=float("inf")), dict(color=(1.0, 1.0)), dict(color=(1.0, float("nan"), 0.0)),
           dict(phong=(0.3, 0.7, 0.4)), dict(phong=(0.3, float("inf"), 0.4, 8.0)), dict(phong=(0.3, 0.7, 0.4, -1.0)),
           dict(refine=17), dict(refine=-1), dict(refine=2.5), dict(skip=2), dict(window=(0, 0, 0, 4)),
           dict(window=(4, 0, 2, 4)), dict(window=(0, 0, 33, 4)), dict(window=(0, 0, 4, 25)), dict(window=(-1, 0, 4, 4)),
           dict(window=(0, 0, 4)), dict(window=(0, 0.5, 4, 4))]
    for kw in bad:
        args = dict(iso=0.5)
        args.update(kw)
        with pytest.raises(ValueError):
            r.isosurface(**args)
    with pytest.raises(ValueError):
        r.pick(32, 0, 0.5)          # outside the image: an empty window


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_node_module_exposes_the_isosurface(native_lib, tmp_path):
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = r"""
const v = require(process.argv[2]);
console.log(JSON.stringify({ methods: Object.getOwnPropertyNames(v.Volxel3DDicomRenderer.prototype),
  natives: [typeof v.native.isosurface, typeof v.native.isoStats], size: v.native.sizeofIsoParams() }));
"""
    (tmp_path / "m.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "m.js"), NAPI], timeout=120))
    from volxel_amd import _abi
    for m in ("isosurface", "pick", "isoStats"):
        assert m in out["methods"]
    assert out["natives"] == ["function", "function"] and out["size"] == C.sizeof(_abi.VxIsoParams)
    dts = open(os.path.join(NAPI, "index.d.ts")).read()
    assert "isosurface(iso: number" in dts and "pick(x: number, y: number, iso: number" in dts and "isoStats()" in dts


# ---- closed forms of the restatement ------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fields():
    from oracle import oracle as O
    return {(k, sp): Field(O, k, SPACINGS[sp]) for k in ("flat", "ramp", "bowl") for sp in SPACINGS}


def _ref(case, fd, **kw):
    p = iso_params(case, fd)
    args = dict(color=COLOUR, phong=case.phong, refine=case.refine)
    args.update(kw)
    return p, IR.isosurface(p, fd.grid, case.iso, **args)


class Model:
    """the isosurface of a case in float64 on the decoded voxels (tier 2).  Per pixel: found, k (the march), the float64 crossing
    x* of the threshold inside the last march step (sample units), the window [x* - e, x* + 2^-refine + e] that s* of a
    bisection must lie in (s* = hi: the crossing lies in the last bracket [hi - 2^-refine, hi], up to e = the fp32 density band
    over the slope along the ray), the normal and its bound.  `clear`: rays whose march decisions (k, n) lie outside the band.

    Variants (negative controls, their s* and normal): unrefined (s* = k), lo (s* = the bracket's lower end), half_plus /
    half_minus (s* +- 1/2), flip (n = +g/|g|), cap_gradient (a cap shaded with the field's gradient instead of -d)."""

    def __init__(self, case, fd, variant=None):
        o, d = field_rays(phong_case(case, fd))
        o = np.broadcast_to(o, d.shape)
        lo_box, hi_box = CF.world_box(fd.ext, fd.spacing, *fd.clip())
        dt, x, n, valid, pos = CF.march_samples(o, d, lo_box, hi_box, fd.ipw, case.step, case.max_steps)
        near, _ = CF.slab(o, d, lo_box, hi_box)
        t0 = near + 0.5 * dt
        q = CF.world_to_index(pos, fd.ext, fd.spacing) - 0.5
        dens = CF.trilinear(fd.dec, *np.moveaxis(q, -1, 0))
        # fp32: positions within four ulps of the largest quantity they are formed from, the density within 2^-20 plus the
        # trilinear's Lipschitz times that
        qabs = float(np.abs(np.where(valid[..., None], q, 0.0)).max()) + 64.0
        self.dq = 4.0 * 2.0 ** -23 * qabs
        self.g = CF.neighbour_steps(fd.dec)
        band = 2.0 ** -20 + float(self.g.sum()) * self.dq
        iso = case.iso
        above = valid & (dens >= iso)
        found = above.any(axis=-1)
        k = np.where(found, above.argmax(axis=-1), 0)
        upto = np.arange(valid.shape[-1]) <= np.where(found, k, n)[..., None]
        amb = (valid & upto & (np.abs(dens - iso) <= band)).any(axis=-1)
        amb |= (np.abs(x - np.round(x)) < 2e-3) & (n < case.max_steps)           # the count n itself in doubt
        cap = found & (k == 0)
        ipos = CF.world_to_index(o, fd.ext, fd.spacing) - 0.5
        idir = d * fd.ipw

        def qs(s):
            return ipos + (t0 + s * dt)[..., None] * idir

        def dens_at(s):
            return CF.trilinear(fd.dec, *np.moveaxis(qs(s), -1, 0))
        # x*: the float64 crossing inside [k - 1, k] (60 bisection steps), and the slope there (the secant of the step, halved:
        # the fields are smooth on one step)
        lo, hi = k - 1.0, k.astype(float)
        d_lo, d_hi = dens_at(lo), dens_at(hi)
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            up = dens_at(mid) >= iso
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        xs = np.where(cap, 0.0, hi)
        slope = 0.5 * np.abs(d_hi - d_lo)
        self.e = np.where(found & ~cap, band / np.maximum(slope, 1e-300), 0.0)
        self.width = np.where(found & ~cap, 2.0 ** -case.refine, 0.0)
        # refine = 0 takes s* = k: the window is [k, k]
        self.xs = np.where(found & ~cap & (case.refine == 0), k.astype(float), xs)
        if case.refine == 0:
            self.e[:] = 0.0
            self.width[:] = 0.0
        self.found, self.k, self.cap, self.clear = found, k, cap, ~amb
        self.o, self.d, self.t0, self.dt, self.n_samples = o, d, t0, dt, n
        self.refine = case.refine
        # the model's s*: the contract's bisection in float64 (the variants move it)
        lo, hi = k - 1.0, k.astype(float)
        for _ in range(case.refine):
            mid = 0.5 * (lo + hi)
            up = dens_at(mid) >= iso
            hi, lo = np.where(up, mid, hi), np.where(up, lo, mid)
        s = np.where(found & ~cap, hi, k.astype(float))
        if variant == "unrefined":
            s = np.where(found & ~cap, k.astype(float), s)
        elif variant == "lo":
            s = np.where(found & ~cap, s - self.width, s)
        elif variant in ("half_plus", "half_minus"):
            s = np.where(found, s + (0.5 if variant == "half_plus" else -0.5), s)
        self.s = s
        _, D = CF.central_differences(fd.dec, qs(s))
        G = D * fd.ipw
        gmag = np.linalg.norm(G, axis=-1)
        shaded = ~cap & ((CF.world_scale(fd.ext, fd.spacing) * gmag) ** 2 > 1e-12)
        grad_n = -G / np.where(gmag > 0, gmag, 1.0)[..., None]
        if variant == "flip":
            grad_n = -grad_n
        use_grad = shaded | (cap & (variant == "cap_gradient") & (gmag > 0))
        self.nrm = np.where(use_grad[..., None], grad_n, -d)
        # the normal's bound: dD_i <= 2^-20 + 2 sum_j g_j dq per axis (two fp32 trilinears at positions off by dq), through
        # |dn| <= 2 |dG| / |G|; the hardware rsq adds 1e-5 (Phong's tolerance).  s* itself lies within the window, a position
        # error of (2^-refine + 2 e) dq_sample: that moves D by at most the same Lipschitz term
        ds = (self.width + 2.0 * self.e) * np.linalg.norm(idir * dt[..., None], axis=-1)
        errG = np.linalg.norm(np.multiply.outer(2.0 ** -20 + 2.0 * float(self.g.sum()) * (self.dq + ds), fd.ipw), axis=-1)
        self.dn = np.where(shaded, np.minimum(2.0, 2.0 * errG / np.maximum(gmag, 1e-300)), 0.0) + 1e-5
        # t and w: the fp32 ray set-up and t = fma(s, dt, t0), w = fma(t, d, o).  t also moves with the ray's origin along d: an
        # orthographic origin comes out of the inverse projection and view in fp32, a few tens of ulps of |o| (measured: 2^-17.4
        # at |o| = 1.05), while w stays on the ray
        self.tol_t = 64.0 * 2.0 ** -23 * (np.abs(o).max(axis=-1) + np.abs(t0) + np.abs(k + 1.0) * dt) + 1e-7
        self.tol_w = 16.0 * 2.0 ** -23 * (np.abs(o).max(axis=-1) + np.abs(t0) + np.abs(k + 1.0) * dt) + 1e-7

    def s_violations(self, s):
        """clear hits whose s* (sample units) lies outside [x* - e, x* + 2^-refine + e]"""
        c = self.clear & self.found
        slack = self.tol_t / self.dt
        out = (s < self.xs - self.e - slack) | (s > self.xs + self.width + self.e + slack)
        return int((c & out).sum())

    def violations(self, hit):
        """the number of clear pixels where a hit buffer breaks this model: the hit flag, s* from t (t = t0 + s* dt in float64,
        within the set-up's rounding) outside its window, or w off the float64 ray at that t"""
        c = self.clear
        f = hit[..., 3] >= 0
        bad = int((c & (f != self.found)).sum())
        both = c & f & self.found
        t = hit[..., 3].astype(np.float64)
        s = (t - self.t0) / self.dt
        bad += self.s_violations(np.where(both, s, self.xs))
        w = self.o + t[..., None] * self.d
        bad += int((both & (np.abs(hit[..., :3] - w).max(axis=-1) > self.tol_w + self.tol_t)).sum())
        return bad

    def normal_violations(self, nrm):
        c = self.clear & self.found
        err = np.linalg.norm(nrm - self.nrm, axis=-1)
        return int((c & (err > self.dn)).sum())


def _ref_normal(case, fd, per):
    """the restatement's normal, from its rule (the same bits as its shading uses): the fp32 central difference, or -d"""
    p = iso_params(case, fd)
    vol = IR.NP.NpVolume(fd.grid)
    hit, n, q0, dq = IR.rays(p)
    o, d, _, _ = IR.world_rays(p)
    s = per["s"]
    q = [IR.fma(s, dq[a], q0[a]) for a in range(3)]
    fl = [np.floor(a) for a in q]
    fr = [a - b for a, b in zip(q, fl)]
    ci = [b.astype(np.int64) for b in fl]
    m = [F32(p.density_transform_inv[i]) for i in (0, 5, 10)]
    scale = F32(p.volume_density_scale)
    g = []
    for a in range(3):
        up = [c + (1 if b == a else 0) for b, c in enumerate(ci)]
        dn = [c - (1 if b == a else 0) for b, c in enumerate(ci)]
        g.append((IR.trilinear_cell(vol, scale, up, fr) - IR.trilinear_cell(vol, scale, dn, fr)) * m[a])
    g = np.stack(g, axis=-1).astype(np.float64)
    g2 = (g * g).sum(axis=-1)
    shaded = ~per["cap"] & (g2 > 1e-12)
    return np.where(shaded[..., None], -g / np.sqrt(np.where(shaded, g2, 1.0))[..., None], -np.stack(d, axis=-1))


@pytest.fixture(scope="module")
def refs(fields):
    out = {}
    for name, case in CASES.items():
        fd = fields[case.kind, case.spacing]
        p, (rgba, hit, counts, per) = _ref(case, fd)
        out[name] = (p, rgba, hit, counts, per, Model(case, fd))
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_reference_meets_the_float64_contract(fields, refs, name):
    """tier 2: on every ray whose decisions lie outside the fp32 band, the hit flag, k and s* equal the float64 march's and t, w
    lie within the fp32 ray set-up's rounding; the normal within its bound; the counters are the march's"""
    case = CASES[name]
    fd = fields[case.kind, case.spacing]
    p, rgba, hit, counts, per, m = refs[name]
    c = m.clear
    assert c.sum() >= 0.75 * c.size, (name, int(c.sum()), c.size)
    assert m.violations(hit) == 0
    assert np.array_equal(per["found"][c], m.found[c])
    assert np.array_equal(per["k"][c & m.found], m.k[c & m.found])
    assert m.s_violations(np.where(per["found"], per["s"].astype(np.float64), m.xs)) == 0
    if case.refine == 0:
        assert np.array_equal(per["s"][c & m.found].astype(np.float64), m.k[c & m.found].astype(np.float64))
    assert m.normal_violations(_ref_normal(case, fd, per)) == 0
    # counters: samples + skipped = k + 1 on a hit, n on a miss; refine per hit that is not a cap
    f = per["found"]
    want = np.where(f, per["k"].astype(np.int64) + 1, per["n"].astype(np.int64))
    assert np.array_equal(per["samples"] + per["skipped"], want)
    assert counts["hits"] == int(f.sum()) and counts["refine_samples"] == case.refine * int((f & ~per["cap"]).sum())
    assert counts["rays"] >= counts["hits"] and counts["skipped"] == 0
    # misses and caps as the contract writes them
    assert (hit[~f] == np.array([0, 0, 0, -1], F32)).all() and (rgba[~f] == 0).all()
    assert (rgba[f][:, 3] == 1).all()
    cap = per["cap"]
    if cap.any():
        o, d, t0, dt = IR.world_rays(p)
        assert np.array_equal(hit[..., 3][cap], t0[cap])
    # each case exercises what its name says
    if "caps" in name:
        assert cap.sum() == f.sum() > 20
    if "misses" in name:
        assert f.sum() == 0 and counts["rays"] > 20 and counts["samples"] == int(per["n"].sum())
    if "maxsteps" in name:
        capped = (m.n_samples >= case.max_steps)
        assert (capped & ~m.found & m.clear).sum() > 10
    if case.kind != "flat":
        assert (f & ~cap).sum() > 5


def _analytic(case, fd, m, hit, per):
    """tier 1: per clear non-cap hit the distance of the hit from the field's surface along the ray, and its bound"""
    sel = m.clear & per["found"] & ~per["cap"]
    w = hit[..., :3].astype(np.float64)
    d = m.d
    eps = fd.eps() + fd.curvature() + float(m.g.sum()) * m.dq + 2.0 ** -20
    if case.kind == "ramp":
        slope = np.abs(fd.b * (d @ RAMP_M))                # density per world unit along the ray
        err = np.abs(fd.f(w) - case.iso) / np.maximum(slope, 1e-300)
    else:
        R = math.sqrt((fd.A - case.iso) / fd.B)
        r = w - fd.c
        rn = np.linalg.norm(r, axis=-1)
        slope = 2.0 * fd.B * np.abs((r * d).sum(axis=-1))     # |df/dt| at the hit
        err = np.abs(rn - R) * (2.0 * fd.B * rn) / np.maximum(slope, 1e-300)
    # the last bracket is dt 2^-refine long; the density error eps moves the crossing by eps / slope
    bound = m.dt * 2.0 ** -case.refine + eps / np.maximum(slope, 1e-300) + m.tol_w
    return sel, err, bound


@pytest.mark.parametrize("name", [n for n in sorted(CASES) if not n.startswith("flat")])
def test_reference_hits_the_analytic_surface(fields, refs, name):
    """tier 1: the ramp's hits lie on the plane f = iso, the bowl's on the sphere |w - c| = sqrt((A - iso) / B), within
    dt 2^-refine + eps / slope (eps the codec's error and the trilinear's curvature term, slope |df/dt| along the ray); the
    normal is -m (ramp) or (w - c) / |w - c| (bowl) within 2 eps |ipw| / |2 grad f| + the fp32 bound"""
    case = CASES[name]
    fd = fields[case.kind, case.spacing]
    p, rgba, hit, counts, per, m = refs[name]
    sel, err, bound = _analytic(case, fd, m, hit, per)
    assert sel.sum() > 5
    assert (err[sel] <= bound[sel]).all(), (float((err / bound)[sel].max()))
    nrm = _ref_normal(case, fd, per)
    w = hit[..., :3].astype(np.float64)
    exact = fd.normal(w)
    q = CF.world_to_index(w, fd.ext, fd.spacing) - 0.5
    true_g = true_grad(fd, q)
    dn = np.minimum(2.0, 2.0 * 2.0 * fd.eps() * np.linalg.norm(fd.ipw) / np.maximum(true_g, 1e-300)) + m.dn
    ok = np.linalg.norm(nrm - exact, axis=-1) <= dn
    assert ok[sel].all(), int((~ok & sel).sum())
    # the colour is Blinn-Phong of that normal (Phong's tolerance)
    light = np.asarray(case.light, float) / np.linalg.norm(case.light)
    h = CF.half_vector(light, m.d)
    want = CF.blinn_phong(np.asarray(COLOUR), nrm, light, h, *case.phong)
    f = per["found"]
    assert np.abs(rgba[..., :3][f] - want[f]).max() <= 1e-5


def test_reference_caps_and_flat_fields(fields, refs):
    """a cap (the ray enters the clip box inside the surface) has s* = 0, t = t0 and n = -d: on the flat field every ray that
    marches caps and is shaded ka + kd max(0, -d.l) + ks max(0, -d.h)^s; above the flat value every ray misses"""
    p, rgba, hit, counts, per, m = refs["flat_iso_caps"]
    case = CASES["flat_iso_caps"]
    f = per["found"]
    assert (per["cap"] == f).all() and (per["s"][f] == 0).all() and counts["refine_samples"] == 0
    assert counts["samples"] == counts["hits"] == int(f.sum())
    light = np.asarray(case.light, float) / np.linalg.norm(case.light)
    h = CF.half_vector(light, m.d)
    want = CF.blinn_phong(np.asarray(COLOUR), -m.d, light, h, *case.phong)
    assert np.abs(rgba[..., :3][f] - want[f]).max() <= 1e-5
    # the ramp's caps: where the entry face lies above the plane
    _, _, _, _, per2, _ = refs["ramp_iso_persp"]
    assert per2["cap"].sum() > 10 and (per2["found"] & ~per2["cap"]).sum() > 10


def test_reference_refine_zero_is_the_sample(refs):
    """refine = 0: s* = k, the first sample at or above iso, exactly"""
    p, rgba, hit, counts, per, m = refs["ramp_iso_r0_step2"]
    f = per["found"]
    assert np.array_equal(per["s"][f], per["k"][f]) and counts["refine_samples"] == 0


def test_reference_range_skipping_keeps_the_hits(fields, native_lib):
    """with the projections' upper bounds, the skipped samples are exactly those whose macro cell lies below iso; the hit buffer
    and the colour are the same bits, and samples + skipped is unchanged per ray"""
    from tests.common import make_scene, small_noise
    from volxel_amd import read_u16_stack_to_grid
    g = read_u16_stack_to_grid(*small_noise(32))
    _, _, _, _, p = make_scene(g, 24, 20, "dvr", cam_pos=(0.3, 0.4, -1.0))
    bound = IR.bound_table(native_lib, g, p)
    for iso in (0.3, 0.6):
        a = IR.isosurface(p, g, iso, refine=6)
        b = IR.isosurface(p, g, iso, refine=6, bound=bound)
        assert np.array_equal(a[1].view(np.uint32), b[1].view(np.uint32))
        assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32))
        assert np.array_equal(a[3]["samples"], b[3]["samples"] + b[3]["skipped"])
        assert b[2]["skipped"] > 0 and a[2]["hits"] > 0


NEGATIVE = {"unrefined": "ramp_iso_persp", "lo": "ramp_aniso_ortho_r4", "half_plus": "bowl_iso_persp",
            "half_minus": "bowl_aniso_ortho", "flip": "bowl_iso_persp", "cap_gradient": "ramp_iso_persp"}


def test_negative_controls_break_the_bound(fields, refs):
    """each wrong float64 model disagrees with the restatement beyond the tier-2 bound on some clear pixel: the restatement (and
    the device, which the GPU tests hold to it bit for bit) would fail these pins if it made the error"""
    for variant, name in NEGATIVE.items():
        case = CASES[name]
        fd = fields[case.kind, case.spacing]
        p, rgba, hit, counts, per, right = refs[name]
        wrong = Model(case, fd, variant=variant)
        wrong.clear = right.clear
        if variant in ("flip", "cap_gradient"):
            nrm = _ref_normal(case, fd, per)
            wrong.dn = right.dn
            bad = wrong.normal_violations(nrm)
            if variant == "cap_gradient":
                assert (per["cap"] & right.clear).sum() > 10
        else:
            bad = right.s_violations(np.where(right.found, wrong.s, right.xs))
        assert bad > 0, variant
