"""Shadowed DVR without a GPU ("light grid"): the ABI of the new field and entry points, both hosts carrying
the setting, and the NumPy restatement (tests/shadow_ref.py) against closed forms."""
import ctypes
import json
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

from oracle import np_oracle as NP
from tests import shadow_ref as SR

from tests.common import NAPI, ROOT
F32 = np.float32


def test_shadow_stride_is_the_last_param_and_matches_the_c_layout(tmp_path):
    from volxel_amd import _abi
    fields = _abi.VxParams._fields_
    assert fields[-1][0] == "dvr_shadow_stride" and fields[-1][1] is ctypes.c_int32
    off = _abi.VxParams.dvr_shadow_stride.offset
    assert off + 4 == ctypes.sizeof(_abi.VxParams)
    src = tmp_path / "sz.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "volxel_hip.h"\n'
                   'int main(void) { printf("%u %u\\n", (unsigned)sizeof(VxParams), '
                   '(unsigned)offsetof(VxParams, dvr_shadow_stride)); return 0; }\n')
    cc = shutil.which("cc") or shutil.which("gcc") or shutil.which("clang")
    if cc is None:
        pytest.skip("no C compiler")
    subprocess.check_call([cc, "-I", os.path.join(ROOT, "include"), str(src), "-o", str(tmp_path / "sz")])
    size, c_off = map(int, subprocess.check_output([str(tmp_path / "sz")]).split())
    assert (size, c_off) == (ctypes.sizeof(_abi.VxParams), off)


def test_shadow_entry_points_are_declared_and_exported(native_lib):
    from volxel_amd import _abi
    names = _abi.declared_symbols("volxel_hip.h")
    for n in ("vx_shadow_stats", "vx_debug_read_shadow_grid"):
        assert n in names
        getattr(native_lib, n)


def test_compute_params_and_viewer_dict_carry_the_stride():
    from volxel_amd import ViewerSettings
    from tests.common import make_scene
    from volxel_amd import synth
    from oracle import oracle as O
    assert ViewerSettings().dvr_shadow_stride == 0
    vox, sp = synth.value_noise(32, seed=3, zero_quantile=0.5)
    g = O.BrickGrid(vox, sp)
    for s in (0, 1, 2, 4):
        st, _, _, _, p = make_scene(g, 8, 8, "dvr", dvr_shadow_stride=s)
        assert p.dvr_shadow_stride == s
        assert st.to_viewer_dict()["dvrShadowStride"] == s


@pytest.mark.skipif(shutil.which("node") is None, reason="node not installed")
def test_javascript_params_block_carries_the_stride(tmp_path, native_lib):
    subprocess.check_call(["make", "-C", NAPI, "-s"])
    script = r"""
const v = require(process.argv[2]);
let captured = null;
v.native.setParams = (ctx, buf) => { captured = buf; };
const r = Object.create(v.Volxel3DDicomRenderer.prototype);
const I = [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1];
r.volume = { transform: I, grid: { transform: I, indexExtent: [16, 16, 16], minMaj: [0, 1] } };
r.densityScale = 1; r.camera = new v.Camera(1); r.width = 8; r.height = 8; r.environment = null; r.envStrength = 1; r.ctx = null;
r.settings = { densityMultiplier: 1, maxSamples: 1, debugHits: false, volumeClipMin: [0, 0, 0], volumeClipMax: [1, 1, 1],
  showEnvironment: false, useEnv: false, lightDir: [0, 0, -1], syncLightDir: false, bounces: 1, gamma: 2.2, exposure: 1,
  sampleRange: [0, 1], renderMode: 'dvr', resolutionFactor: 1, dvrStepVoxels: 0.5, dvrErtEpsilon: 1e-4, dvrJitter: false,
  dvrMaxSteps: 1024, dvrSkipEmpty: true, phong: [0.3, 0.7, 0.4, 32], dvrShadowStride: 2 };
r.bindUniforms();
const dv = new DataView(captured);
console.log(JSON.stringify({ size: captured.byteLength, last: dv.getInt32(captured.byteLength - 4, true),
  methods: Object.getOwnPropertyNames(v.Volxel3DDicomRenderer.prototype), natives: [typeof v.native.shadowStats, typeof v.native.readShadowGrid] }));
"""
    (tmp_path / "p.js").write_text(script)
    out = json.loads(subprocess.check_output(["node", str(tmp_path / "p.js"), NAPI], timeout=120))
    from volxel_amd import _abi
    assert out["size"] == ctypes.sizeof(_abi.VxParams) and out["last"] == 2
    assert "shadowStats" in out["methods"] and "readShadowGrid" in out["methods"]
    assert out["natives"] == ["function", "function"]


def _slab_scene(stride=1, res=(4, 4), clip_z=(0.0, 1.0)):
    """48 x 16 x 16 voxels (padded to 64^3): a receiver plate x in [8, 12), an occluder x in [32, 48), density 1 there and 0 elsewhere (every
    voxel decodes to exactly 0 or 1); a TF of constant alpha with sample range [0.5, 1] (a sample counts where its trilinear
    density is >= 0.5); the light toward +x in index space; an orthographic camera looking along the z axis at the receiver"""
    from tests.common import make_scene
    from oracle import oracle as O
    vox = np.zeros((16, 16, 48), dtype=np.uint16)
    vox[:, :, 8:12] = 1000
    vox[:, :, 32:48] = 1000
    g = O.BrickGrid(vox, (1.0, 1.0, 1.0))
    st, cam, vol, ds, p = make_scene(g, res[0], res[1], "dvr", dvr_skip_empty=False, show_environment=False, use_env=False,
                                     clip_min=(0.0, 0.0, clip_z[0]), clip_max=(1.0, 1.0, clip_z[1]),
                                     sample_range=(0.5, 1.0), dvr_shadow_stride=stride)
    m = np.asarray(p.density_transform_inv[:], dtype=F32).reshape(4, 4)   # column major: m[col][row]
    assert np.count_nonzero(m[:3, :3] - np.diag(np.diag(m[:3, :3]))) == 0 and (np.diag(m[:3, :3]) > 0).all()
    p.light_dir[0], p.light_dir[1], p.light_dir[2] = -1.0, 0.0, 0.0   # toward the light: -light_dir = +x
    alpha = 0.05
    tf = np.tile(np.array([1.0, 0.8, 0.6, alpha], dtype=F32), 16)
    return g, p, tf, 16, alpha


def _hand_count(p, grid, stride, i):
    """samples of the light march from node x index i (interior y, z) whose density is >= 0.5, counted with a scalar loop over
    the sample positions along x: voxel values are 0 / 1, so the density at cell-frame x is the linear blend of its two voxels"""
    idir, dt, lo, hi, n = SR.light_march(p, grid.index_extent, stride)
    ox = F32(stride * i + 0.5)
    assert idir[1] == 0 and idir[2] == 0 and idir[0] > 0
    near = max(F32(0), (lo[0] - ox) / idir[0])
    far = (hi[0] - ox) / idir[0]
    if not near <= far:
        return 0, dt
    t0 = NP.fma(F32(0.5), dt, near)
    ns = int(np.ceil((far - t0) / dt)) if (far - t0) / dt > 0 else 0
    vals = np.zeros(int(grid.index_extent[0]) + 2)
    vals[8:12] = 1.0
    vals[32:48] = 1.0
    count = 0
    for m in range(ns):
        qx = float(NP.fma(F32(m), dt * idir[0], NP.fma(t0, idir[0], ox) - F32(0.5)))
        c = math.floor(qx)
        f = qx - c
        d = (vals[c] if c >= 0 else 0.0) * (1 - f) + (vals[c + 1] if c + 1 >= 0 else 0.0) * f
        assert abs(d - 0.5) > 1e-3, "a sample on the threshold: the count would depend on rounding"
        count += d >= 0.5
    return count, dt


@pytest.mark.parametrize("stride", [1, 2])
def test_reference_light_grid_meets_the_closed_form(stride):
    g, p, tf, L, alpha = _slab_scene(stride)
    T, samples = SR.light_grid(p, g, tf, L, stride)
    assert samples > 0
    maj = float(p.volume_maj)
    for i in range(T.shape[2]):
        n, dt = _hand_count(p, g, stride, i)
        want = math.exp(-n * alpha * maj * float(dt))
        hi = 14 // stride + 1
        got = T[1:hi, 1:hi, i]      # nodes inside the plates in y and z (the data spans y, z in [0, 16))
        assert np.allclose(got, want, rtol=2e-5, atol=0), (i, n, float(got.min()), float(got.max()), want)
    # the receiver (x ~ 9..11) sits in the occluder's shadow, the far side of the occluder is lit
    assert T[4, 4, 9 // stride] < 0.5 and T[4, 4, -1] == 1.0


def test_reference_receiver_ratio_is_the_light_transmittance():
    """an orthographic camera looking along z at the receiver plate: every sample of a pixel has the same x, hence the same
    T_L, so shadowed / unshadowed = T_L at that x.  The clip box ends inside the plates in z (index z in [2, 14]): samples near
    its faces take the outermost node inside it, whose T_L is the same"""
    g, p, tf, L, alpha = _slab_scene(1, res=(4, 4), clip_z=(2 / 64, 14 / 64))
    from volxel_amd import Camera  # noqa: F401  (make_scene built the camera)
    # look straight down the z axis at the receiver: ortho camera over x in [8, 12) voxels, y in [6, 10)
    M = np.asarray(p.density_transform[:], dtype=np.float64).reshape(4, 4).T    # index -> world, row major
    def world(ix, iy, iz):
        return (M @ np.array([ix, iy, iz, 1.0]))[:3]
    c = world(10.0, 8.0, 40.0)
    half = world(12.0, 10.0, 40.0) - c
    view_inv = np.eye(4)
    view_inv[:3, 3] = c
    proj_inv = np.diag([half[0], half[1], 0.0, 1.0])
    p.camera_ortho = 1
    for k in range(16):
        p.camera_view_inv[k] = float(view_inv.T.reshape(-1)[k])
        p.camera_proj_inv[k] = float(proj_inv.T.reshape(-1)[k])
    T, _ = SR.light_grid(p, g, tf, L, 1)
    plain, n0, t0 = SR.dvr_image_shadowed(p, g, tf, L)
    shad, n1, t1 = SR.dvr_image_shadowed(p, g, tf, L, T, 1)
    assert (n0, t0) == (n1, t1) and n0 > 0
    ref, nref = NP.dvr_image(p, g, tf, L)
    assert nref == n0 and np.array_equal(plain, ref)   # with T_L = 1 the restatement is np_oracle's DVR, bit for bit
    ratio = shad[..., 0] / plain[..., 0]
    W = p.res[0]
    for px in range(W):
        # the pixel's x (index): its cell-frame x lies between nodes; T_L is linear in x between them and constant in y, z
        x_idx = 8.0 + (px + 0.5) * 4.0 / W
        q = x_idx - 0.5
        i0 = int(math.floor(q))
        f = q - i0
        n_a, _ = _hand_count(p, g, 1, i0)
        n_b, dt = _hand_count(p, g, 1, i0 + 1)
        maj = float(p.volume_maj)
        want = (1 - f) * math.exp(-n_a * alpha * maj * float(dt)) + f * math.exp(-n_b * alpha * maj * float(dt))
        assert np.allclose(ratio[:, px], want, rtol=1e-4), (px, ratio[:, px], want)
    assert (ratio < 0.9).all()
