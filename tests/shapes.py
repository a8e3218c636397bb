"""Volumes, masks and fields built by hand, and the cases on them that more than one test file uses: the segment volumes
(serpentine, tube, the stack with odd sides, the diagonal chains), the masks that cross brick faces, edges and corners, the
renderer shell and the struct-offset probe of the host tests, and the flat / ramp / bowl fields of the Phong and isosurface pins
with their scene cases."""
import os
import shutil
import subprocess

import numpy as np
import pytest

from tests import closed_form as CF
from tests import segedit_ref as ER
from tests import segment_ref as SG
from tests.common import F32, F32_MAX, ROOT, make_scene


# ---- the segment volumes --------------------------------------------------------------------------------------------------------
def serpentine():
    """a one-voxel-wide path: rows along x at every other y, joined at alternating ends, in every other z layer, the layers
    joined at the end of their last row; no two parts of it closer than 2 voxels except along the path, so it is one path under
    6 and 26 alike, and it crosses brick faces hundreds of times"""
    X, Y, Z = 48, 40, 16
    v = np.zeros((Z, Y, X), dtype=np.uint16)
    x = 0
    rows, layers = list(range(0, Y, 2)), list(range(0, Z, 2))
    for li, z in enumerate(layers):
        order = rows if li % 2 == 0 else rows[::-1]
        for ri, y in enumerate(order):
            xe = X - 1 if x == 0 else 0
            v[z, y, min(x, xe):max(x, xe) + 1] = 3000
            x = xe
            if ri + 1 < len(order):
                v[z, (y + order[ri + 1]) // 2, x] = 3000
        if li + 1 < len(layers):
            v[z + 1, order[-1], x] = 3000
    return v, (1.0, 1.0, 1.0)


def tube():
    """1040 x 16 x 24: a noisy tube along x through 130 bricks, with noise below the threshold around it"""
    X, Y, Z = 1040, 16, 24
    z, y, x = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing="ij")
    r2 = (y - 7.5 - 3 * np.sin(x / 40.0)) ** 2 + (z - 11.5 - 4 * np.cos(x / 55.0)) ** 2
    rng = np.random.default_rng(5)
    v = np.where(r2 < 16, 2500, 600) + rng.integers(0, 300, size=r2.shape)
    return v.astype(np.uint16), (0.5, 0.5, 0.8)


def odd():
    """a 37 x 29 x 45 stack: the builder pads it to 40 x 32 x 48 (index_extent is always 8 x the brick grid, so no brick is
    partial), and the padding is part of the volume the segment runs over"""
    from volxel_amd import synth
    v, _ = synth.value_noise(48, seed=3, zero_quantile=0.3)
    return np.ascontiguousarray(v[:45, :29, :37]), (1.0, 1.2, 0.9)


# (volume, seed rule, lo, hi, box): lo / hi as quantiles of d ("q0.6") or values; seed: the voxel of the largest d in the
# predicate, or a fixed voxel
CASES = {
    "noise_q60": ("noise", "max", "q0.6", None, None),     # small_noise is half zeros: q0.5 would be lo = 0, the whole volume
    "noise_q70": ("noise", "max", "q0.7", None, None),
    "noise_q90": ("noise", "max", "q0.9", None, None),
    "noise_band": ("noise", "max", "q0.6", "q0.95", ((3, 0, 5), (60, 50, 63))),
    "phantom_bone": ("phantom", "max", 0.75, None, None),
    "phantom_air": ("phantom", (0, 0, 0), 0.0, 0.05, None),
    "odd": ("odd", "max", "q0.55", None, None),
    "serpentine": ("serpentine", (0, 0, 0), "half", None, None),
    "tube": ("tube", (0, 8, 12), "half", None, None),
}


def resolve(d, seed, lo, hi, box):
    def val(v):
        if v is None:
            return F32_MAX
        if isinstance(v, str) and v.startswith("q"):
            return float(np.quantile(d, float(v[1:])))
        if v == "half":
            return float(d.max()) / 2
        return float(v)
    lo_v, hi_v = val(lo), val(hi)
    p = SG.predicate(d, lo_v, hi_v, box)
    if seed == "max":
        dd = np.where(p, d, -np.inf)
        z, y, x = np.unravel_index(int(np.argmax(dd)), d.shape)
        seed = (int(x), int(y), int(z))
    return seed, lo_v, hi_v, p


# one-voxel chains whose only links are diagonal (no two voxels share a face), 40 long in a 40^3 volume (5 bricks a side): each
# step of a chain changes two or three coordinates at once, and 39 = 8 * 5 - 1 makes the reversed coordinate cross a brick
# boundary at the same step as the others.  So every brick-to-brick step is across a brick edge (two coordinates) or a brick
# corner (three), never a face: only the 12 edge and 8 corner directions of the 26-flood can follow them.  The seed is the
# middle voxel, so the flood runs both ways and each chain uses both opposite directions of its edge / corner.
CHAINS = {
    "corner+++": lambda k: (k, k, k), "corner+-+": lambda k: (k, 39 - k, k), "corner-++": lambda k: (39 - k, k, k),
    "corner++-": lambda k: (k, k, 39 - k),
    "edge_xy++": lambda k: (k, k, 20), "edge_xy+-": lambda k: (k, 39 - k, 20),
    "edge_xz++": lambda k: (k, 20, k), "edge_xz+-": lambda k: (k, 20, 39 - k),
    "edge_yz++": lambda k: (20, k, k), "edge_yz+-": lambda k: (20, k, 39 - k),
}


# ---- masks ----------------------------------------------------------------------------------------------------------------------
def shape_of(g):
    X, Y, Z = (int(e) for e in g.index_extent)
    return (Z, Y, X)


def same_stats(s, mask, d):
    st = SG.stats(mask, d)
    assert s.count == st["count"] and s.bbox_lo == st["bbox_lo"] and s.bbox_hi == st["bbox_hi"], (s, st)
    assert F32(s.d_min) == F32(st["d_min"]) and F32(s.d_max) == F32(st["d_max"]), (s, st)
    assert abs(s.d_sum - st["d_sum"]) <= 1e-9 * abs(st["d_sum"]), (s.d_sum, st["d_sum"])
    assert s.converged


def uploaded_shapes(shape):
    """shapes that cross brick faces, edges and corners and touch all six faces of the volume: blobs (wrapped noise), cubes in
    two opposite corners of the volume, a box around the brick corner (8, 8, 8), a diagonal chain through brick corners, a
    hollow shell across several bricks and a one-voxel plate on the brick face z = 16"""
    Z, Y, X = shape
    m = ER.blobs(shape, seed=11, sigma=2.0, q=0.8)
    m[:3, :3, :3] = True
    m[Z - 4:, Y - 4:, X - 4:] = True
    m[6:11, 6:11, 6:11] = True
    for k in range(min(shape) - 2):
        m[k + 1, k, k] = True
    m |= ER.shell(shape, (13, 5, 19), (27, 26, 37))
    m[16, 9:23, 3:X - 2] = True
    for a in range(3):   # all six faces
        assert m.take(0, axis=a).any() and m.take(-1, axis=a).any()
    return m


# ---- host tests without a device ------------------------------------------------------------------------------------------------
def offsets(tmp_path, name, fields):
    src = tmp_path / f"{name}.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "volxel_hip.h"\n'
                   'int main(void) { printf("%u' + " %u" * len(fields) + '\\n", (unsigned)sizeof(' + name + ')'
                   + "".join(f", (unsigned)offsetof({name}, {n})" for n in fields) + "); return 0; }\n")
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / name)])
    return [int(x) for x in subprocess.check_output([str(tmp_path / name)]).split()]


def renderer_shell(ext=(16, 16, 24)):
    from volxel_amd import Volxel3DRenderer
    from volxel_amd.scene import Grid, Volume
    r = Volxel3DRenderer.__new__(Volxel3DRenderer)
    r._ctx = None
    r.volume = Volume(Grid(min_maj=(0.0, 1.0), index_extent=np.asarray(ext, float), transform=np.eye(4)))
    return r


# ---- the fields of the Phong and isosurface pins ------------------------------------------------------------------------------
FIELD_RES = (40, 30)
SPACINGS = {"iso": (1.0, 1.0, 1.0), "aniso": (0.5, 0.75, 1.25)}
DIMS = (21, 29, 33)                     # z, y, x: ragged, padded to a 64^3 index extent
VMAX = 4095


def _normalised(v):
    v = np.asarray(v, float)
    return v / np.linalg.norm(v)


def _ext(spacing):
    return (64, 64, 64)


def _data_world(spacing):
    """(centre, half extent) of the data's box in world space"""
    ext = _ext(spacing)
    lo = CF.index_to_world(np.zeros(3), ext, spacing)
    hi = CF.index_to_world(np.array(DIMS[::-1], float), ext, spacing)
    return 0.5 * (lo + hi), 0.5 * (hi - lo)


RAMP_M = _normalised((0.48, -0.6, 0.64))


class Field:
    """a field given in world space, its u16 stack (code VMAX = density 1) and the oracle's decoded voxels"""

    def __init__(self, oracle, kind, spacing):
        self.kind, self.spacing = kind, np.asarray(spacing, float)
        self.ext = _ext(spacing)
        self.ipw = CF.index_per_world(spacing, self.ext)
        self.c, _ = _data_world(spacing)
        z, y, x = np.meshgrid(*[np.arange(n) for n in DIMS], indexing="ij")
        w = CF.index_to_world(np.stack([x + 0.5, y + 0.5, z + 0.5], axis=-1), self.ext, spacing)
        if kind == "flat":
            ideal = np.full(DIMS, 0.5)
            vox = np.full(DIMS, 2000, np.uint16)
            vox[-1, -1, -1] = 4000
            self.grid = oracle.BrickGrid(vox, tuple(spacing))
            self.ideal = ideal
            self.dec = CF.decode(oracle, self.grid)
            self.cut = 0.25
            self.margin = (9, 9, 9)             # voxels: keeps the gradient taps clear of the brick of the brighter corner
            return
        if kind == "ramp":
            self.b = 0.4 / float(np.abs((w - self.c) @ RAMP_M).max())
            self.cut = 0.5                      # the iso-plane through the data's centre
        else:
            # the ball f >= cut has world radius R, R - 2 voxels inside the data on every axis; f stays positive to 1.6 R
            self.R = float(((np.array(DIMS[::-1]) / 2.0 - 3.0) / self.ipw).min())
            self.A, self.B, self.cut = 0.95, 0.35 / self.R ** 2, 0.6
        self.ideal = self.f(w)
        assert self.ideal.min() > 0.0 if kind == "ramp" else True
        self.grid = oracle.BrickGrid(np.round(np.clip(self.ideal, 0.0, 1.0) * VMAX).astype(np.uint16), tuple(spacing),
                                     max_value=VMAX)
        self.dec = CF.decode(oracle, self.grid)
        self.margin = (2, 2, 2)

    def f(self, w):
        if self.kind == "ramp":
            return 0.5 + self.b * ((w - self.c) @ RAMP_M)
        return self.A - self.B * ((w - self.c) ** 2).sum(axis=-1)

    def normal(self, w):
        """the exact outward normal -grad f / |grad f|"""
        if self.kind == "ramp":
            return np.broadcast_to(-RAMP_M, w.shape)
        r = w - self.c
        return r / np.maximum(np.linalg.norm(r, axis=-1, keepdims=True), 1e-300)

    def clip(self):
        """the clip box as fractions of the index extent: the data with `margin` voxels off every face (taps included)"""
        d = np.array(DIMS[::-1], float)
        m = np.array(self.margin, float)
        if self.kind == "bowl":          # the ball and 1.5 voxels around it
            lo = self.c - (self.R + 1.5 / self.ipw)
            hi = self.c + (self.R + 1.5 / self.ipw)
            return tuple(CF.world_to_index(lo, self.ext, self.spacing) / 64.0), tuple(CF.world_to_index(hi, self.ext, self.spacing) / 64.0)
        return tuple(m / 64.0), tuple((d - m) / 64.0)

    def eps(self):
        """the codec's voxel error over the data: max |decode - ideal|"""
        nz, ny, nx = DIMS
        return float(np.abs(self.dec[:nz, :ny, :nx] - np.round(np.clip(self.ideal, 0, 1) * VMAX) / VMAX).max()
                     + 0.5 / VMAX)

    def curvature(self):
        """the trilinear's largest error on the field, sum_a a_a / 4, a_a the index-space quadratic coefficient"""
        if self.kind != "bowl":
            return 0.0
        return float((self.B / self.ipw ** 2).sum() / 4.0)


class Case:
    def __init__(self, field, eye_off, light, phong, step=0.5, alpha=0.08, ortho=None, max_steps=1 << 20, ert_eps=1e-4,
                 env=False, look_off=(0.0, 0.0, 0.0), inside=False):
        self.look = field.c + np.asarray(look_off, float)
        # inside: the eye sits at eye_off from the data's centre, inside the clip box
        self.eye = (field.c if inside else self.look) + np.asarray(eye_off, float)
        if light is None:      # the light shines toward the camera from a little off the view axis
            light = -_normalised(-_normalised(eye_off) + np.array([0.12, 0.06, 0.0]))
        self.field, self.light = field, _normalised(light)
        self.phong, self.step, self.alpha, self.ortho = phong, step, alpha, ortho
        self.max_steps, self.ert_eps, self.env = max_steps, ert_eps, env
        self.inside = inside


def field_rays(case):
    if case.ortho is None:
        (d,), _ = CF.camera_rays(case.eye, case.look, *FIELD_RES)
        return np.broadcast_to(case.eye, d.shape), d
    return CF.ortho_rays(case.eye, case.look, *FIELD_RES, case.ortho)


def true_grad(fd, q):
    """|2 grad_w f| in units of D ipw: the ramp's 2 b, the bowl's 4 B |w - c| (the device's D = 2 df/dindex)"""
    w = CF.index_to_world(q + 0.5, fd.ext, fd.spacing)
    if fd.kind == "ramp":
        return 2.0 * fd.b * np.ones(q.shape[:-1])
    if fd.kind == "bowl":
        return 4.0 * fd.B * np.linalg.norm(w - fd.c, axis=-1)
    return np.zeros(q.shape[:-1])


def field_params(case, mode, skip=False):
    fd = case.field
    lo, hi = fd.clip()
    _, _, _, _, p = make_scene(fd.grid, *FIELD_RES, mode, cam_pos=tuple(case.eye), look_at=tuple(case.look), clip_min=lo,
                               clip_max=hi, ortho=case.ortho, show_environment=case.env, use_env=False,
                               light_dir=tuple(case.light), dvr_step_voxels=case.step, dvr_max_steps=case.max_steps,
                               dvr_ert_epsilon=case.ert_eps, dvr_jitter=False, dvr_skip_empty=skip,
                               sample_range=(fd.cut, 1.0), phong=case.phong)
    return p


# the isosurface pins: their cases on the fields above
ISO_COLOUR = (0.8, 0.5, 0.3)
ISO_PHONG = (0.3, 0.7, 0.4, 32.0)
L_OBL = (-0.4, -0.75, 0.53)


class IsoCase:
    def __init__(self, kind, spacing, iso, eye_off, refine=8, step=0.5, ortho=None, max_steps=1 << 20, light=L_OBL,
                 phong=ISO_PHONG):
        self.kind, self.spacing, self.iso, self.eye_off = kind, spacing, iso, eye_off
        self.refine, self.step, self.ortho, self.max_steps = refine, step, ortho, max_steps
        self.light, self.phong = light, phong


ISO_CASES = {
    "ramp_iso_persp": IsoCase("ramp", "iso", 0.5, (0.3, 0.25, -0.6)),
    "ramp_aniso_ortho_r4": IsoCase("ramp", "aniso", 0.45, (-0.2, 0.3, -0.6), refine=4, step=0.25, ortho=0.25),
    "ramp_iso_r0_step2": IsoCase("ramp", "iso", 0.55, (0.35, -0.2, -0.55), refine=0, step=2.0),
    "ramp_aniso_maxsteps": IsoCase("ramp", "aniso", 0.6, (0.3, 0.25, -0.6), max_steps=12),
    "ramp_iso_r16": IsoCase("ramp", "iso", 0.5, (-0.3, -0.25, -0.6), refine=16),
    "bowl_iso_persp": IsoCase("bowl", "iso", 0.6, (0.3, 0.25, -0.6)),
    "bowl_aniso_ortho": IsoCase("bowl", "aniso", 0.7, (-0.25, 0.3, -0.6), step=0.125, ortho=0.12),
    "bowl_aniso_r2": IsoCase("bowl", "aniso", 0.55, (0.5, 0.1, -0.4), refine=2),
    "flat_iso_caps": IsoCase("flat", "iso", 0.25, (0.3, 0.25, -0.6)),
    "flat_aniso_misses": IsoCase("flat", "aniso", 0.75, (0.3, 0.25, -0.6), ortho=0.3),
}


def phong_case(case, fd):
    return Case(fd, case.eye_off, case.light, case.phong, step=case.step, ortho=case.ortho, max_steps=case.max_steps)


def iso_params(case, fd):
    return field_params(phong_case(case, fd), "dvr")
