"""Shared scene builders for the tests (CPU and GPU).  A new feature's test file starts from this module, tests/shapes.py and
tests/js_host.py, never from another test file.  Nothing here touches a device or loads the library at import."""
import ctypes as C
import os

import numpy as np

from volxel_amd import ViewerSettings, compute_params, synth
from volxel_amd.scene import Camera, Grid, Volume, from_flat
from volxel_amd.transfer import default_transfer_function, generate_transfer_function
from volxel_amd.settings import BENCHMARK_SETTINGS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAPI = os.path.join(ROOT, "volxel_amd", "napi")
F32 = np.float32
F32_MAX = float(np.finfo(np.float32).max)
LAYOUTS = {"brickf32": 2, "bricku8": 4, "reference": 0, "cellquad": 1, "auto": 3}   # a file that covers fewer selects from it


def make_scene(grid, width, height, mode="dvr", cam_pos=(0.0, 0.0, -1.0), look_at=(0, 0, 0),
               clip_min=(0, 0, 0), clip_max=(1, 1, 1), env=False, ortho=None, **kw):
    """env=True: uniforms as the viewer binds them with an environment map resident (use_env = 1);
    ortho=h: [build] orthographic camera of half height h (BASELINE config 1) instead of the reference's
    perspective camera"""
    s = ViewerSettings(render_mode=mode, bounces=kw.pop("bounces", 1),
                       volume_clip_min=clip_min, volume_clip_max=clip_max, **kw)
    cam = Camera(1)
    cam.pos = np.asarray(cam_pos, dtype=np.float64)
    cam.view = np.asarray(look_at, dtype=np.float64)
    cam.ortho_half_height = ortho
    vol = Volume(Grid(tuple(grid.min_maj), np.asarray(grid.index_extent, float), from_flat(grid.transform)))
    ds = vol.normalise()
    p = compute_params(s, cam, vol, ds, width, height, has_environment=env)
    return s, cam, vol, ds, p


def benchmark_tf():
    colors = BENCHMARK_SETTINGS["transfer"]["transfer"]["colors"]
    return generate_transfer_function(colors)


BENCH_CAM = dict(cam_pos=BENCHMARK_SETTINGS["other"]["cameraPos"],
                 look_at=BENCHMARK_SETTINGS["other"]["cameraLookAt"])


def small_noise(n=64, seed=7):
    """small 3-octave noise volume with empty space, for parity cases"""
    v, sp = synth.value_noise(n, seed=seed, zero_quantile=0.5)
    return v, sp


def oracle_grid(vox, sp=(1.0, 1.0, 1.0)):
    """the oracle's own brick grid of a u16 stack (no device, no product preprocessor)"""
    from oracle import oracle as O
    return O.BrickGrid(vox, sp)


def default_environment(oracle):
    """the viewer's default map (environment.ts:102-130) as the oracle's Environment"""
    from volxel_amd import Environment
    e = Environment.default()
    return oracle.Environment(e.floats, e.width, e.height)


# ---- the GPU side: renderers on a grid ------------------------------------------------------------------------------------------
def grid(vox, sp=(1, 1, 1)):
    from volxel_amd import read_u16_stack_to_grid
    return read_u16_stack_to_grid(vox, sp)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def renderer(g, layout=None, devices=None, mode="dvr", size=(64, 48), **settings):
    """a renderer on g with the benchmark settings restored, then render_mode, then `settings` in the order given"""
    from volxel_amd import Volxel3DRenderer
    r = Volxel3DRenderer(size[0], size[1], device=None if devices else 0, layout=layout, devices=devices)
    r.setup_from_grid(g)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.render_mode = mode
    for k, v in settings.items():
        setattr(r.settings, k, v)
    return r


def frame(r, frames=1, in_flight=1):
    """accumulation and counters restarted, then `frames` frames: (accum, counters)"""
    r.restart_rendering()
    r.reset_counters()
    r.render(frames=frames, in_flight=in_flight)
    return r.read_accum(), r.counters()


def upload_volume(lib, ctx, g):
    """vx_upload_volume through the C ABI alone"""
    u3 = lambda t: (C.c_uint32 * 3)(*[int(x) for x in t])
    ind = np.ascontiguousarray(g.indirection, dtype=np.uint32)
    rng = np.ascontiguousarray(g.range, dtype=np.uint16)
    atl = np.ascontiguousarray(g.atlas, dtype=np.uint8)
    mips = [np.ascontiguousarray(m, dtype=np.uint16) for m, _ in g.range_mipmaps]
    ptrs = (C.c_void_p * len(mips))(*[m.ctypes.data for m in mips])
    sizes = (C.c_uint32 * (3 * len(mips)))(*[int(x) for _, s in g.range_mipmaps for x in s])
    return lib.vx_upload_volume(ctx, ind.ctypes.data, u3(g.indirection_size), rng.ctypes.data, u3(g.range_size),
                                atl.ctypes.data, u3(g.atlas_size), len(mips), ptrs, C.cast(sizes, C.c_void_p),
                                u3(g.index_extent))


_D = {}


def densities(name, g, p):
    """segment_ref.densities of the volume `name` under p's scale, computed once per session"""
    from tests import segment_ref as SG
    key = (name, float(p.volume_density_scale), float(p.volume_inv_maj))
    if key not in _D:
        _D[key] = SG.densities(g, p.volume_density_scale, p.volume_inv_maj)
    return _D[key]


def segment_volumes():
    """the five volumes of the segment, edit, islands and mesh tests"""
    from tests import shapes
    return {"noise": grid(*small_noise(64)), "phantom": grid(*synth.ct_phantom(64)), "odd": grid(*shapes.odd()),
            "serpentine": grid(*shapes.serpentine()), "tube": grid(*shapes.tube())}
