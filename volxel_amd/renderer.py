"""Host-side mirror of the reference's render core (volxel-3d-viewer/src/viewer.ts) above
the C ABI of libvolxel_hip.so.

`Volxel3DRenderer` keeps the names of the reference class `Volxel3DDicomRenderer`
(viewer.ts:111) for the calls on the hot path:

    setup_from_grid(grid)          viewer.ts:1080-1145   (setupFromGrid)
    change_transfer_func(data, n)  viewer.ts:1147-1153   (changeTransferFunc)
    restart_rendering()            viewer.ts:1155-1181   (frameIndex = 0)
    bind_uniforms()                viewer.ts:1295-1357   (+ scene.ts:53-56)
    render()                       viewer.ts:1183-1293   (one accumulation sample)
    restore_settings(json)         viewer.ts:704-713
    render_mode (property)         viewer.ts:1442-1452

Everything that touches pixels goes through the HIP library; there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from dataclasses import dataclass

import numpy as np

from . import _abi
from .scene import Camera, Grid, Volume, flat, from_flat
from .environment import Environment
from .settings import ViewerSettings, verify_settings
from .transfer import default_transfer_function, generate_transfer_function
from .mesh import Mesh, check_extract_args

LOW_RESOLUTION_DURATION = 5  # viewer.ts:132


class VolxelError(RuntimeError):
    """What viewer.ts:797-816 handleError receives."""


def sample_weight(frame_index: int, low_res_duration: int = LOW_RESOLUTION_DURATION) -> float:
    """viewer.ts:1356."""
    if frame_index < low_res_duration:
        return 0.0
    return (frame_index - low_res_duration) / (frame_index - low_res_duration + 1)


def compute_params(settings: ViewerSettings, camera: Camera, volume: Volume, density_scale: float,
                   width: int, height: int, env_strength: float = 1.0, shard_rank: int = 0,
                   shard_count: int = 1, has_environment: bool = False) -> "_abi.VxParams":
    """bindUniforms (viewer.ts:1295-1357) + Camera.bindAsUniforms (scene.ts:53-56):
    doubles on the host, rounded to float32 on upload."""
    p = _abi.VxParams()

    def put(name, arr):
        a = np.asarray(arr, dtype=np.float64).astype(np.float32).reshape(-1)
        getattr(p, name)[:] = a.tolist()

    view = camera.view_matrix()
    proj = camera.proj_matrix(width / height)
    view32 = from_flat(flat(view).astype(np.float32))  # the shader only sees the f32 upload
    proj32 = from_flat(flat(proj).astype(np.float32))
    put("camera_view", flat(view))
    put("camera_proj", flat(proj))
    put("camera_view_inv", flat(np.linalg.inv(view32)))   # inverse(camera_view), utils.glsl:24
    put("camera_proj_inv", flat(np.linalg.inv(proj32)))   # inverse(camera_proj), utils.glsl:29
    p.camera_ortho = 1 if camera.ortho_half_height is not None else 0   # [build] BASELINE config 1

    mn, maj = volume.min_maj()
    lo, hi = volume.aabb_clipped(settings.volume_clip_min, settings.volume_clip_max)
    put("volume_aabb_min", lo)
    put("volume_aabb_max", hi)
    mult = settings.density_multiplier
    p.volume_min = mn * density_scale * mult                 # viewer.ts:1321
    p.volume_maj = maj * density_scale * mult                # viewer.ts:1322
    p.volume_inv_maj = 1.0 / (maj * density_scale * mult)    # viewer.ts:1323
    put("volume_albedo", [0.9, 0.9, 0.9])                    # viewer.ts:1325
    p.volume_phase_g = 0.0                                   # viewer.ts:1326
    p.volume_density_scale = density_scale * mult            # viewer.ts:1327
    combined = volume.combined_transform()
    put("density_transform", flat(combined))                 # viewer.ts:1330
    put("density_transform_inv", flat(np.linalg.inv(combined)))  # viewer.ts:1331
    put("sample_range", settings.sample_range)               # viewer.ts:1343

    put("light_dir", settings.light_dir)                     # viewer.ts:1303
    p.env_strength = env_strength                            # environment.ts:83
    p.show_environment = 1 if settings.show_environment else 0   # viewer.ts:1338
    # viewer.ts:1340; an environment map must be resident (the viewer always has the default one)
    p.use_env = 1 if (settings.use_env and has_environment) else 0
    p.bounces = int(settings.bounces)                        # viewer.ts:1339
    p.res[0], p.res[1] = int(width), int(height)             # viewer.ts:1353 (quirk Q2 dropped)
    p.debug_hits = 1 if settings.debug_hits else 0           # viewer.ts:1354
    p.render_mode = _abi.RENDER_MODES[settings.render_mode]

    p.dvr_step_voxels = settings.dvr_step_voxels
    p.dvr_ert_tau = -math.log(settings.dvr_ert_epsilon)
    p.dvr_jitter = 1 if settings.dvr_jitter else 0
    p.dvr_max_steps = int(settings.dvr_max_steps)
    p.dvr_skip_empty = 1 if settings.dvr_skip_empty else 0
    p.dvr_shadow_stride = int(settings.dvr_shadow_stride)
    # K = albedo * mis * f_p * Le / pdf for the directional light (fragment.frag:94-97,
    # environment.glsl:30-33, utils.glsl:104,121-124), in float32 like the shader
    f32 = np.float32
    inv_4pi = f32(1.0) / (f32(4.0) * f32(math.pi))
    f_p = inv_4pi * (f32(1.0) - f32(0.0)) / (f32(1.0) * f32(1.0))
    mis = (f32(1.0) / (f32(1.0) + f_p * f_p)) if settings.show_environment else f32(1.0)
    le = f32(env_strength) * f32(4.01)
    gain = ((f32(0.9) * mis) * f_p) * le
    put("dvr_gain", [gain, gain, gain])
    p.phong_ka, p.phong_kd, p.phong_ks, p.phong_shininess = [float(x) for x in settings.phong]
    p.shard_rank, p.shard_count = int(shard_rank), int(shard_count)
    return p


_worker_factory = None
COMPONENTS = {}


def register_volxel_components(worker_factory=None):
    """registerVolxelComponents (viewer.ts:1455-1462): remembers the worker factory and registers the component
    classes under the reference's element names.  The four widget elements (slider, histogram viewer, cube direction,
    colour ramp) are browser UI and have no counterpart here; `volxel-3d-viewer` maps to the renderer class.  The
    factory is kept for hosts that run the preprocessor elsewhere: the renderer itself calls the native preprocessor
    in-process."""
    global _worker_factory
    _worker_factory = worker_factory
    COMPONENTS["volxel-3d-viewer"] = Volxel3DRenderer
    return COMPONENTS


@dataclass(frozen=True)
class Segment:
    """What Volxel3DRenderer.segment returns (VxSegmentResult): the voxel count, the inclusive bbox (x, y, z), min / max / sum
    (float64) / mean of the density over the segment (0, 0, 0 and nan when empty), the flood's rounds and brick visits (which may
    vary from run to run), whether it converged, and its volume: volume_grid = count * |det(grid.transform[:3, :3])| in the
    grid's own units (the voxel spacing: mm^3 for DICOM), volume_world = count * |det(density_transform[:3, :3])| in the
    scene's, where the volume is normalised to a unit box."""
    count: int
    bbox_lo: tuple
    bbox_hi: tuple
    d_min: float
    d_max: float
    d_sum: float
    mean: float
    rounds: int
    converged: bool
    brick_visits: int
    volume_grid: float
    volume_world: float


@dataclass(frozen=True)
class IslandSegment(Segment):
    """The `Segment` of the mask after keep_largest_islands / remove_small_islands / keep_island_at, with the op's own
    figures (VxIslandsResult): `islands` of the mask before the op, `kept` after it, `largest` = the voxel count of the
    largest island before the op (0 for an empty mask)."""
    islands: int = 0
    kept: int = 0
    largest: int = 0


class Islands:
    """What Volxel3DRenderer.islands returns: the islands of the current segment in canonical order (count descending, ties by
    the C-order index of the anchor ascending; island k has label k + 1).  count: how many; sizes: their voxel counts (uint64);
    table: one dict per island (label, count, anchor, bbox_lo, bbox_hi, each (x, y, z)); largest; segment: the `Segment` of the
    labelled mask; labels(): the dense (Z, Y, X) uint32 label volume, read from the device when asked (refused once the
    segment has changed)."""

    def __init__(self, renderer, res, rows, segment):
        self._renderer = renderer
        self.count = int(res.islands)
        self.largest = int(res.largest)
        self.segment = segment
        self.sizes = np.array([r.count for r in rows], dtype=np.uint64)
        self.table = [dict(label=int(r.label), count=int(r.count), anchor=tuple(r.anchor[:]), bbox_lo=tuple(r.bbox_lo[:]),
                           bbox_hi=tuple(r.bbox_hi[:])) for r in rows]

    def labels(self) -> np.ndarray:
        return self._renderer.island_labels()

    def __len__(self):
        return self.count


class Volxel3DRenderer:
    """Headless counterpart of the `<volxel-3d-viewer>` element's render core."""

    def __init__(self, width: int = 1920, height: int = 1080, device: int | None = None,
                 shard_rank: int = 0, shard_count: int = 1, layout: int | None = None,
                 low_res_preview: bool = False, devices=None):
        """width, height: the canvas.  low_res_preview=True reproduces the viewer's interactive
        ramp (viewer.ts:1167-1188): after every restart the first `low_resolution_duration` frames
        are rendered at 0.33 x the canvas and shown NEAREST-magnified; a headless caller that wants
        full-size frames from frame 0 (tests, bench.py) leaves it off.
        device: the HIP ordinal (None = 0).  devices: render one image on several GPUs of this process instead
        (vx_create_group: member i renders shard i, a device may repeat); excludes `device` and shard_count != 1."""
        self._ctx = None
        if devices is not None:
            devices = [int(d) for d in devices]
            if device is not None:
                raise ValueError("pass either device or devices, not both")
            if shard_count != 1 or shard_rank != 0:
                raise ValueError("a device group deals the shards itself: devices excludes shard_rank / shard_count")
            if not 1 <= len(devices) <= 64:
                raise ValueError(f"devices must name 1 to 64 GPUs, not {len(devices)}")
        self._lib = _abi.load_library()
        ctx = C.c_void_p()
        if devices is None:
            rc = self._lib.vx_create(0 if device is None else int(device), C.byref(ctx))
        else:
            ids = (C.c_int * len(devices))(*devices)
            rc = self._lib.vx_create_group(ids, len(devices), C.byref(ctx))
        if rc != 0:
            msg = self._lib.vx_last_error(None)
            raise VolxelError(msg.decode() if msg else f"vx_create failed ({rc})")
        self._ctx = ctx
        self.devices = devices                        # None: one context on one device
        self.settings = ViewerSettings()
        self.camera = Camera(1)                       # viewer.ts:418
        self.volume: Volume | None = None
        self.density_scale = 1.0
        self.environment: Environment | None = None
        self._env_strength = 1.0
        self.frame_index = 0
        self.canvas_width, self.canvas_height = int(width), int(height)
        self.width, self.height = int(width), int(height)      # current render size
        self.shard_rank, self.shard_count = shard_rank, shard_count
        self.low_resolution_duration = LOW_RESOLUTION_DURATION
        self.low_res_preview = bool(low_res_preview)
        self.tile_order = None                                 # vx_set_tile_order permutation, if any
        self.resolution_factor = 1.0                           # viewer.ts:131, the ramp state
        if layout is not None:
            self._check(self._lib.vx_set_layout(self._ctx, int(layout)))
        self._check(self._lib.vx_resize(self._ctx, self.width, self.height))
        self.set_environment(Environment.default())   # viewer.ts:372-374
        data, length = default_transfer_function()    # viewer.ts:377-385
        self.change_transfer_func(data, length)

    # -- error contract (viewer.ts:797-816) -------------------------------------------
    def _check(self, rc):
        if rc != 0:
            raise VolxelError(self._lib.vx_last_error(self._ctx).decode())

    def close(self):
        if getattr(self, "_ctx", None):
            self._lib.vx_destroy(self._ctx)
            self._ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- viewer.ts:1442-1452 ------------------------------------------------------------
    @property
    def render_mode(self) -> str:
        return self.settings.render_mode

    @render_mode.setter
    def render_mode(self, to: str):
        if to not in _abi.RENDER_MODES:
            raise VolxelError(f"Unrecognized render mode provided: {to}")
        self.settings.render_mode = to
        self.restart_rendering()

    # -- viewer.ts:963-975 restartFromFiles (+ worker.ts:77-104: files -> bytes -> read_dicoms_to_grid)
    def restart_from_files(self, files, n_threads: int = 0):
        """files: DICOM slices as paths or bytes objects, in stacking order (the reference does not
        sort them either, lib.rs:150-176).  ZIP / URL variants are container I/O outside the path."""
        from .preprocessor import read_dicoms_to_grid
        blobs = []
        for f in files:
            if isinstance(f, (bytes, bytearray, memoryview)):
                blobs.append(bytes(f))
            else:
                with open(f, "rb") as fh:
                    blobs.append(fh.read())
        self.setup_from_grid(read_dicoms_to_grid(blobs, n_threads))

    # -- viewer.ts:977-1017: the other load methods.  The reference posts the bytes to its worker, which decodes
    #    them (worker.ts:60-76,105-126); here the host decodes what the Python standard library can (containers.py)
    def restart_from_zip(self, zip_file, n_threads: int = 0):
        """restartFromZip (viewer.ts:977-989): a ZIP of DICOM slices as bytes or a path; folder rule of zip.rs:54-70"""
        from .containers import read_zip_slices
        from .preprocessor import read_dicoms_to_grid
        if not isinstance(zip_file, (bytes, bytearray, memoryview)):
            with open(zip_file, "rb") as fh:
                zip_file = fh.read()
        self.setup_from_grid(read_dicoms_to_grid(read_zip_slices(zip_file), n_threads))

    def restart_from_zip_url(self, url: str, n_threads: int = 0):
        """restartFromZipUrl (viewer.ts:991-1003, worker.ts:115-118)"""
        from .containers import fetch_bytes
        self.restart_from_zip(fetch_bytes(url), n_threads)

    def restart_from_urls(self, urls, n_threads: int = 0):
        """restartFromURLs (viewer.ts:1005-1017, worker.ts:120-123): one DICOM slice per URL, in the order given"""
        from .containers import fetch_bytes
        self.restart_from_files([fetch_bytes(u) for u in urls], n_threads)

    def load_env(self, data):
        """loadEnv (viewer.ts:1019-1033, worker.ts:77-90, hdr.rs:23-36): an encoded environment map.  Radiance RGBE is
        decoded; OpenEXR raises (decode it elsewhere and call setup_env with the floats)."""
        from .containers import decode_environment
        try:
            floats, w, h = decode_environment(data)
        except ValueError as e:
            raise VolxelError(str(e)) from None
        self.setup_env({"floats": floats, "width": w, "height": h})

    def load_env_from_url(self, url: str):
        """loadEnvFromUrl (viewer.ts:1035-1040)"""
        from .containers import fetch_bytes
        self.load_env(fetch_bytes(url))

    # -- viewer.ts:443-449,543-551,789-795: the light follows the camera ("backlight") ---------
    def maybe_sync_light(self):
        """maybeSyncLight (viewer.ts:789-795): lightDir = -(view - pos); assigning it to the direction widget
        (cubeDirection.ts:177-206) normalises it and hands the unit vector back through the 'direction' event
        (viewer.ts:536-541), so the uniform of the next frame is the unit vector from the look-at point to the camera.
        As in the reference, restoring a settings file does NOT re-aim the light (viewer.ts:696-713 never calls it):
        the file's lightDir is used until the camera is rotated or the toggle changes."""
        if self.settings.sync_light_dir:
            d = np.asarray(self.camera.pos, dtype=np.float64) - np.asarray(self.camera.view, dtype=np.float64)
            n = float(np.linalg.norm(d))
            if n > 0.0:                                    # the widget ignores a zero vector (cubeDirection.ts:187-190)
                self.settings.light_dir = (float(d[0] / n), float(d[1] / n), float(d[2] / n))

    def rotate_camera(self, by):
        """the canvas drag of viewer.ts:443-449: orbit, re-aim the synced light, restart"""
        self.camera.rotate_around_view(by)
        self.maybe_sync_light()
        self.restart_rendering()

    @property
    def sync_light_dir(self) -> bool:
        return bool(self.settings.sync_light_dir)

    @sync_light_dir.setter
    def sync_light_dir(self, on: bool):               # the backlight toggle, viewer.ts:543-551
        self.settings.sync_light_dir = bool(on)
        self.maybe_sync_light()
        self.restart_rendering()

    # -- viewer.ts:1073-1078 setupEnv(WasmWorkerMessageEnvReturn) -----------------------------
    def setup_env(self, env_message):
        """env_message: mapping / object with width, height, floats (row 0 = top)"""
        g = (lambda k: env_message[k]) if isinstance(env_message, dict) else (lambda k: getattr(env_message, k))
        # a new Environment starts at strength 1 (environment.ts:15)
        self.set_environment(Environment(g("floats"), int(g("width")), int(g("height")), 1.0))

    # -- viewer.ts:1080-1145 ------------------------------------------------------------
    def setup_from_grid(self, grid):
        """grid: preprocessor.BrickGridMessage (= WasmWorkerMessageDicomReturn)."""
        self.density_scale = 1.0
        self.settings.volume_clip_max = (1.0, 1.0, 1.0)
        self.settings.volume_clip_min = (0.0, 0.0, 0.0)
        g = Grid(min_maj=tuple(grid.min_maj), index_extent=np.asarray(grid.index_extent, float),
                 transform=from_flat(grid.transform))
        self.volume = Volume(g)
        self.density_scale *= self.volume.normalise()
        u3 = lambda t: (C.c_uint32 * 3)(*[int(x) for x in t])
        ind = np.ascontiguousarray(grid.indirection, dtype=np.uint32)
        rng = np.ascontiguousarray(grid.range, dtype=np.uint16)
        atl = np.ascontiguousarray(grid.atlas, dtype=np.uint8)
        n = len(grid.range_mipmaps)
        mips = [np.ascontiguousarray(m, dtype=np.uint16) for m, _ in grid.range_mipmaps]
        # the C ABI takes raw pointers and cannot check lengths: the arrays must hold what the size fields say
        prod = lambda t: int(t[0]) * int(t[1]) * int(t[2])
        if ind.size < prod(grid.indirection_size):
            raise VolxelError("setup_from_grid: indirection shorter than indirection_size")
        if rng.size < 2 * prod(grid.range_size):
            raise VolxelError("setup_from_grid: range shorter than 2 * range_size")
        if atl.size < prod(grid.atlas_size):
            raise VolxelError("setup_from_grid: atlas shorter than atlas_size")
        for m, (_, st) in zip(mips, grid.range_mipmaps):
            if m.size < 2 * prod(st):
                raise VolxelError("setup_from_grid: range mipmap shorter than 2 * stride")
        mip_ptrs = (C.c_void_p * max(n, 1))(*[m.ctypes.data for m in mips])
        mip_sizes = (C.c_uint32 * (3 * max(n, 1)))(*[int(x) for _, s in grid.range_mipmaps for x in s])
        self._check(self._lib.vx_upload_volume(
            self._ctx, ind.ctypes.data, u3(grid.indirection_size), rng.ctypes.data,
            u3(grid.range_size), atl.ctypes.data if atl.size else None, u3(grid.atlas_size), n,
            mip_ptrs, C.cast(mip_sizes, C.c_void_p), u3(grid.index_extent)))
        self.restart_rendering()

    # -- viewer.ts:1147-1153 ------------------------------------------------------------
    def change_transfer_func(self, data, length: int):
        a = np.ascontiguousarray(data, dtype=np.float32).reshape(-1)
        if a.size != 4 * length:
            raise VolxelError("transfer function must hold length*4 floats")
        self._check(self._lib.vx_upload_transfer(self._ctx, a.ctypes.data, int(length)))
        self._tf = (a.copy(), int(length))
        self.frame_index = 0

    def set_color_stops(self, colors, steps: int = 128):
        data, length = generate_transfer_function(colors, steps)
        self.change_transfer_func(data, length)

    # -- viewer.ts:1073-1078 setupEnv --------------------------------------------------------
    def set_environment(self, env: "Environment | None"):
        """env = None removes the map: use_env then falls back to the directional light."""
        if env is None:
            self._check(self._lib.vx_upload_environment(self._ctx, None, 0, 0))
        else:
            self._check(self._lib.vx_upload_environment(self._ctx, env.floats.ctypes.data, env.width, env.height))
        self.environment = env
        self.restart_rendering()

    @property
    def env_strength(self) -> float:                  # environment.ts:15 `strength`
        return self.environment.strength if self.environment is not None else self._env_strength

    @env_strength.setter
    def env_strength(self, v: float):
        self._env_strength = float(v)
        if self.environment is not None:
            self.environment.strength = float(v)

    # -- viewer.ts:1155-1181 ------------------------------------------------------------
    def restart_rendering(self):
        if self.low_res_preview:                               # viewer.ts:1176-1178
            self.resolution_factor = 0.33
            self._resize_framebuffers_to_canvas()
        self.frame_index = 0

    def _resize_framebuffers_to_canvas(self):                  # viewer.ts:925-949
        f = self.resolution_factor * self.settings.resolution_factor if self.low_res_preview else 1.0
        w = max(1, math.floor(self.canvas_width * f))
        h = max(1, math.floor(self.canvas_height * f))
        if (w, h) != (self.width, self.height):
            self.width, self.height = w, h
            self._check(self._lib.vx_resize(self._ctx, w, h))
            self.tile_order = None   # a dealing order belongs to one tile grid; the library dropped it too

    def resize(self, width: int, height: int):
        if int(width) <= 0 or int(height) <= 0:
            self._check(self._lib.vx_resize(self._ctx, max(0, int(width)), max(0, int(height))))  # raises
        self.canvas_width, self.canvas_height = int(width), int(height)
        self._resize_framebuffers_to_canvas()
        self.restart_rendering()

    # -- viewer.ts:704-713 restoreSettings ---------------------------------------------
    def restore_settings(self, s: dict):
        verify_settings(s)
        t = s["transfer"]
        self.settings.density_multiplier = t["densityMultiplier"]
        self.settings.sample_range = tuple(t["histogramRange"])          # viewer.ts:650
        if t["transfer"]["type"] == "color_stops":
            self.set_color_stops(t["transfer"]["colors"])
        else:
            rows = np.asarray(t["transfer"]["colors"], dtype=np.float32)
            self.change_transfer_func(rows.reshape(-1), rows.shape[0])
        d = s["display"]
        self.settings.bounces = d["bounces"]
        self.settings.max_samples = d["samples"]
        self.settings.gamma, self.settings.exposure = d["gamma"], d["exposure"]
        self.settings.debug_hits = d["debugHits"]
        self.settings.render_mode = d["renderMode"]
        self.settings.resolution_factor = d["resolutionFactor"]
        l = s["lighting"]
        self.settings.show_environment = l["showEnv"]
        self.settings.use_env = l["useEnv"]
        self.env_strength = l["envStrength"]
        self.settings.sync_light_dir = l["syncLightDir"]
        self.settings.light_dir = tuple(l["lightDir"])
        o = s["other"]
        self.settings.volume_clip_max = tuple(o["clipMax"])
        self.settings.volume_clip_min = tuple(o["clipMin"])
        self.camera.pos = np.asarray(o["cameraPos"], dtype=np.float64)
        self.camera.view = np.asarray(o["cameraLookAt"], dtype=np.float64)
        self.restart_rendering()

    # -- viewer.ts:1295-1357 ------------------------------------------------------------
    def bind_uniforms(self):
        if self.volume is None:
            raise VolxelError("Trying to bind uniforms without a volume.")
        p = compute_params(self.settings, self.camera, self.volume, self.density_scale, self.width,
                           self.height, self.env_strength, self.shard_rank, self.shard_count,
                           has_environment=self.environment is not None)
        self._check(self._lib.vx_set_params(self._ctx, C.byref(p)))
        self._params = p
        return p

    # -- viewer.ts:1183-1293 ------------------------------------------------------------
    def render(self, frames: int = 1, rebind: bool = True, in_flight: int = 32):
        """Render `frames` accumulation samples (the body of render() while
        frameIndex <= maxSamples).  Asynchronous; call finish() or a read_* to wait.
        Up to `in_flight` frames go into one launch (vx_render_frames): same bits as one launch per frame
        (in_flight=1), 1.6x the speed at 32."""
        if self.low_res_preview and (self.frame_index < self.low_resolution_duration or self.resolution_factor != 1.0):
            # the ramp changes the framebuffer size at frame low_resolution_duration: step up to it
            while frames > 0 and self.frame_index <= self.settings.max_samples:
                if self.frame_index >= self.low_resolution_duration:
                    if self.resolution_factor != 1.0:          # viewer.ts:1185-1188
                        self.resolution_factor = 1.0
                        self._resize_framebuffers_to_canvas()
                    break
                self.bind_uniforms()
                self._check(self._lib.vx_render_frame(self._ctx, self.frame_index, 0.0))
                self.frame_index += 1
                frames -= 1
            if frames == 0:
                return
            rebind = True
        if rebind:
            self.bind_uniforms()
        if in_flight > 1 and frames > 1:
            n = max(0, min(frames, self.settings.max_samples + 1 - self.frame_index))
            if n:
                w = (C.c_float * n)(*[sample_weight(self.frame_index + i, self.low_resolution_duration)
                                      for i in range(n)])
                self._check(self._lib.vx_render_frames(self._ctx, self.frame_index, n, w, int(in_flight)))
                self.frame_index += n
            return
        for _ in range(frames):
            if self.frame_index > self.settings.max_samples:     # viewer.ts:1194
                break
            w = sample_weight(self.frame_index, self.low_resolution_duration)
            self._check(self._lib.vx_render_frame(self._ctx, self.frame_index, w))
            self.frame_index += 1

    def finish(self):  # gl.finish(), viewer.ts:1289
        self._check(self._lib.vx_finish(self._ctx))

    def read_accum(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 4), dtype=np.float32)
        self._check(self._lib.vx_read_accum(self._ctx, out.ctypes.data))
        return out

    def read_display(self) -> np.ndarray:  # blit pass to the canvas, viewer.ts:1253-1265
        out = np.empty((self.canvas_height, self.canvas_width, 4), dtype=np.uint8)
        self._check(self._lib.vx_read_display_scaled(self._ctx, out.ctypes.data, self.canvas_width,
                                                     self.canvas_height, float(self.settings.exposure),
                                                     float(self.settings.gamma)))
        return out

    # -- viewer.ts:856-890,1213-1252: the data-benchmark-url runner ------------------------
    def start_benchmark(self, collection: dict, volumes: dict | None = None, progress=None) -> list:
        """Run a VolxelBenchmark collection (public/benchmark.json) and return the list of
        VolxelBenchmarkResult records the viewer would hand to saveBenchmark.

        Per entry, as startBenchmark/singleBenchmark do: optional volume switch, restoreSettings,
        renderMode, restart; then frames 0..maxSamples are rendered one by one with gl.finish()
        (vx_finish) inside the timed region, on the viewer's framebuffer sizing (resolutionFactor and
        the 0.33 preview for the first frames).  `volumes` maps an entry's "zip" string to a brick
        grid message (ZIP/DICOM container I/O is outside the path); entries without one keep the
        current volume.  Times are milliseconds like performance.now()."""
        import datetime
        import os
        import platform
        import time
        from .settings import verify_benchmark
        verify_benchmark(collection)
        name, cus, mem = self.device_info()
        device = {"platform": platform.platform(), "userAgent": "volxel_amd " + self._lib.vx_version().decode(),
                  "deviceMemory": mem / 2 ** 30, "hardwareConcurrency": os.cpu_count(),
                  "screen": {"width": self.canvas_width, "height": self.canvas_height, "pixelRatio": 1},
                  "gpu": {"vendor": "AMD", "renderer": name.strip(), "version": "HIP",
                          "shadingLanguageVersion": "gfx950", "supportedExtensions": [], "computeUnits": cus}}
        results = []
        saved_preview = self.low_res_preview
        self.low_res_preview = True
        try:
            for entry in collection["benchmarks"]:
                if entry.get("zip") is not None:
                    if not volumes or entry["zip"] not in volumes:
                        raise VolxelError(f"benchmark volume not provided: {entry['zip']}")
                    self.setup_from_grid(volumes[entry["zip"]])
                if entry.get("env") is not None:
                    raise VolxelError("benchmark entry asks for an environment map URL; pass the decoded "
                                      "map with set_environment() before the run")
                st = entry["settings"]
                self.restore_settings(collection["sharedSettings"][st] if isinstance(st, int) else st)
                if entry.get("renderMode"):
                    self.render_mode = entry["renderMode"]
                self.restart_rendering()
                total = 0.0
                while self.frame_index <= self.settings.max_samples:      # viewer.ts:1194
                    t0 = time.perf_counter()
                    self.render(1)
                    self.finish()                                         # viewer.ts:1213-1218
                    total += (time.perf_counter() - t0) * 1e3
                    if progress and self.frame_index % 100 == 0:
                        progress(entry.get("name"), self.frame_index, self.settings.max_samples)
                rf = self.settings.resolution_factor
                results.append({
                    "name": entry.get("name"), "settings": self.settings.to_viewer_dict(),
                    "timePerSample": total / self.frame_index, "totalTime": total,
                    "viewport": [0, 0, rf * self.canvas_width, rf * self.canvas_height],
                    "device": device,
                    "timestamp": datetime.datetime.now(datetime.timezone.utc).isoformat().replace("+00:00", "Z"),
                })
        finally:
            self.low_res_preview = saved_preview
            if not saved_preview:
                self.resolution_factor = 1.0
                self._resize_framebuffers_to_canvas()
        return results

    # -- measurement hooks (viewer.ts:1213-1252 benchmark harness) -----------------------
    def counters(self):
        c = _abi.VxCounters()
        self._check(self._lib.vx_get_counters(self._ctx, C.byref(c)))
        return c

    def reset_counters(self):
        self._check(self._lib.vx_reset_counters(self._ctx))

    def last_launch_blocks(self):
        """(march, miss): the 16x16-pixel blocks per frame the last render launch gave its march kernel and the light kernel
        of the blocks that cannot hit the clip box (vx_debug_last_launch_blocks; miss = 0: the launch was not split)"""
        a, b = C.c_uint32(), C.c_uint32()
        self._check(self._lib.vx_debug_last_launch_blocks(self._ctx, C.byref(a), C.byref(b)))
        return a.value, b.value

    def set_stream(self, hip_stream: int | None):
        self._check(self._lib.vx_set_stream(self._ctx, C.c_void_p(hip_stream or 0)))

    def set_layout(self, layout: int):
        self._check(self._lib.vx_set_layout(self._ctx, int(layout)))

    def upload_stats(self):
        """(seconds, host bytes, pinned) of the last volume upload: copies from pinned host memory in chunks,
        device-side layout build overlapped behind them (viewer.ts:1106-1142 is its texImage3D counterpart)"""
        s, b, pin = C.c_double(), C.c_uint64(), C.c_int()
        self._check(self._lib.vx_upload_stats(self._ctx, C.byref(s), C.byref(b), C.byref(pin)))
        return s.value, b.value, bool(pin.value)

    def shadow_stats(self):
        """(builds, light_samples, last_build_ms) of the light grid of shadowed DVR (settings.dvr_shadow_stride): builds since
        the renderer was created, light-march samples and HIP-event time of the last build"""
        b, n, ms = C.c_uint64(), C.c_uint64(), C.c_double()
        self._check(self._lib.vx_shadow_stats(self._ctx, C.byref(b), C.byref(n), C.byref(ms)))
        return b.value, n.value, ms.value

    def read_shadow_grid(self) -> np.ndarray:
        """the last light grid built, shape (nz, ny, nx): transmittance toward the light at node (i, j, k), cell-frame
        position stride * (i, j, k)"""
        dims = (C.c_uint32 * 3)()
        self._check(self._lib.vx_debug_read_shadow_grid(self._ctx, None, dims))
        out = np.empty((dims[2], dims[1], dims[0]), dtype=np.float32)
        self._check(self._lib.vx_debug_read_shadow_grid(self._ctx, out.ctypes.data, dims))
        return out

    def slice(self, sp, reduce: str = "mean", display: str | None = None, window=None):
        """A slice or thick slab of the volume (vx_slice; planes from volxel_amd.mpr).  reduce: "mean", "max" or "min" over the
        sp.slab_samples samples; display: None, "grey" (window = (value shown black, value shown white)) or "tf" (the transfer
        function, premultiplied by its alpha).  Binds the current uniforms first (the densities use their density scale).
        Returns the (H, W) float32 values, row 0 = y = 0, or (values, the (H, W, 4) uint8 display) when a display is asked."""
        if not isinstance(sp, _abi.VxSliceParams):
            raise TypeError("sp must be a VxSliceParams (volxel_amd.mpr builds them)")
        if reduce not in _abi.SLICE_REDUCE:
            raise ValueError(f"reduce must be one of {sorted(_abi.SLICE_REDUCE)}, not {reduce!r}")
        if display not in _abi.SLICE_DISPLAY:
            raise ValueError(f"display must be None, 'grey' or 'tf', not {display!r}")
        q = _abi.VxSliceParams.from_buffer_copy(sp)
        W, H, N = int(q.size[0]), int(q.size[1]), int(q.slab_samples)
        if not (1 <= W <= _abi.SLICE_MAX_SIZE and 1 <= H <= _abi.SLICE_MAX_SIZE):
            raise ValueError(f"slice size must be 1 .. {_abi.SLICE_MAX_SIZE} per side, not {W} x {H}")
        if not 1 <= N <= _abi.SLICE_MAX_SAMPLES:
            raise ValueError(f"slab_samples must be 1 .. {_abi.SLICE_MAX_SAMPLES}, not {N}")
        for name in ("origin", "du", "dv", "dn"):
            if not np.isfinite(np.asarray(getattr(q, name)[:], dtype=np.float32)).all():
                raise ValueError(f"slice {name} must be finite")
        if display == "grey":
            w = np.asarray(window if window is not None else (), dtype=np.float64).reshape(-1)
            if w.size != 2 or not np.isfinite(w.astype(np.float32)).all() or not np.float32(w[1]) > np.float32(w[0]):
                raise ValueError(f"display 'grey' needs window = (black, white) with black < white, not {window!r}")
            q.window[0], q.window[1] = float(w[0]), float(w[1])
        elif window is not None:
            raise ValueError("window applies to display 'grey' only")
        q.reduce = _abi.SLICE_REDUCE[reduce]
        q.display = _abi.SLICE_DISPLAY[display]
        self.bind_uniforms()
        values = np.empty((H, W), dtype=np.float32)
        rgba = np.empty((H, W, 4), dtype=np.uint8) if display is not None else None
        self._check(self._lib.vx_slice(self._ctx, C.byref(q), values.ctypes.data,
                                       rgba.ctypes.data if rgba is not None else None))
        return values if rgba is None else (values, rgba)

    def slice_stats(self):
        """(samples, kernel_ms) of the last slice: W * H * slab_samples and its HIP-event time"""
        n, ms = C.c_uint64(), C.c_double()
        self._check(self._lib.vx_slice_stats(self._ctx, C.byref(n), C.byref(ms)))
        return n.value, ms.value

    def isosurface(self, iso: float, color=(1.0, 1.0, 1.0), phong=None, refine: int = 8, skip: bool = True, window=None):
        """The shaded first-hit isosurface d = iso of the current view (vx_isosurface, DESIGN.md section 2 "Isosurfaces"): DVR's
        rays and samples, `refine` bisection steps, Blinn-Phong on `color` with phong = (ka, kd, ks, shininess) (default: the
        settings' phong).  skip: range skipping (same bits).  window = (x0, y0, x1, y1) of the render size (x0 <= x < x1, GL rows:
        y = 0 is the bottom row) or None for the whole image.  Binds the current uniforms first.  Returns (rgba, hit), both
        (h, w, 4) float32 over the window, row 0 = y0: rgba alpha 1 on a hit and all 0 on a miss; hit = (world x, y, z, t) or
        (0, 0, 0, -1) on a miss."""
        q = _abi.VxIsoParams()
        iso32 = np.float32(iso)
        if not np.isfinite(iso32):
            raise ValueError(f"iso must be finite, not {iso!r}")
        col = np.asarray(color, dtype=np.float64).reshape(-1)
        if col.size != 3 or not np.isfinite(col.astype(np.float32)).all():
            raise ValueError(f"color must be three finite values, not {color!r}")
        ph = np.asarray(self.settings.phong if phong is None else phong, dtype=np.float64).reshape(-1)
        if ph.size != 4 or not np.isfinite(ph.astype(np.float32)).all():
            raise ValueError(f"phong must be four finite values (ka, kd, ks, shininess), not {phong!r}")
        if ph[3] < 0:
            raise ValueError(f"shininess must be >= 0, not {ph[3]}")
        if isinstance(refine, bool) or int(refine) != refine or not 0 <= int(refine) <= _abi.ISO_MAX_REFINE:
            raise ValueError(f"refine must be an integer 0 .. {_abi.ISO_MAX_REFINE}, not {refine!r}")
        if skip not in (True, False, 0, 1):
            raise ValueError(f"skip must be True or False, not {skip!r}")
        W, H = int(self.width), int(self.height)
        if window is None:
            x0, y0, x1, y1 = 0, 0, W, H
        else:
            w = tuple(window)
            if len(w) != 4 or any(isinstance(a, bool) or int(a) != a for a in w):
                raise ValueError(f"window must be four integers (x0, y0, x1, y1), not {window!r}")
            x0, y0, x1, y1 = (int(a) for a in w)
            if not (0 <= x0 < x1 <= W and 0 <= y0 < y1 <= H):
                raise ValueError(f"window {window!r} is empty or outside the render size {W} x {H}")
        q.iso = float(iso32)
        q.color[0], q.color[1], q.color[2] = (float(a) for a in col)
        q.ka, q.kd, q.ks, q.shininess = (float(a) for a in ph)
        q.refine = int(refine)
        q.skip = 1 if skip else 0
        q.window[0], q.window[1], q.window[2], q.window[3] = x0, y0, x1, y1
        self.bind_uniforms()
        rgba = np.empty((y1 - y0, x1 - x0, 4), dtype=np.float32)
        hit = np.empty((y1 - y0, x1 - x0, 4), dtype=np.float32)
        self._check(self._lib.vx_isosurface(self._ctx, C.byref(q), rgba.ctypes.data, hit.ctypes.data))
        return rgba, hit

    def pick(self, x: int, y: int, iso: float, refine: int = 16):
        """the world point (x, y, z) where the ray of pixel (x, y) (GL rows: y = 0 is the bottom row) first reaches density iso,
        or None when it misses: a one-pixel isosurface window"""
        _, hit = self.isosurface(iso, refine=refine, window=(x, y, x + 1, y + 1))
        h = hit[0, 0]
        return None if h[3] < 0 else tuple(float(a) for a in h[:3])

    def iso_stats(self):
        """(rays, hits, samples, refine_samples, skipped, kernel_ms) of the last isosurface"""
        v = [C.c_uint64() for _ in range(5)]
        ms = C.c_double()
        self._check(self._lib.vx_iso_stats(self._ctx, *[C.byref(a) for a in v], C.byref(ms)))
        return tuple(a.value for a in v) + (ms.value,)

    def segment(self, seed, lo: float, hi: float = math.inf, connectivity: int = 6, box=None, max_rounds: int = 0):
        """Seeded region growing (vx_segment, DESIGN.md section 2 "Segmentation"): the connected component of
        lo <= d(i) <= hi (both inclusive; d(i) = (volume_density_scale * v(i)) * volume_inv_maj, the isosurfaces' density at
        q = i) inside `box` that holds the voxel `seed` = (x, y, z).  connectivity: 6 (faces) or 26 (faces, edges, corners).
        box = ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices, or None for the whole volume.  hi = inf stands for the
        largest float32.  max_rounds: a cap on the flood's rounds (0: no practical cap); a capped flood returns
        converged = False and a connected part of the segment.  Binds the current uniforms first.  Returns a `Segment`; the
        mask stays on the device (segment_mask, slice_mask) until the next segment or upload."""
        if self.volume is None:
            raise VolxelError("segment: no volume (setup_from_grid first)")
        ext = [int(e) for e in self.volume.grid.index_extent]
        q = _abi.VxSegmentParams()
        sd = tuple(seed)
        if len(sd) != 3 or any(isinstance(a, bool) or int(a) != a for a in sd):
            raise ValueError(f"seed must be three integer voxel indices (x, y, z), not {seed!r}")
        if not all(0 <= int(a) < e for a, e in zip(sd, ext)):
            raise ValueError(f"seed {seed!r} is outside the index extent {tuple(ext)}")
        lo32 = np.float32(lo)
        hi32 = np.float32(np.finfo(np.float32).max) if hi == math.inf else np.float32(hi)
        if not (np.isfinite(lo32) and np.isfinite(hi32)):
            raise ValueError(f"lo and hi must be finite (hi may be inf), not {lo!r}, {hi!r}")
        if lo32 > hi32:
            raise ValueError(f"lo = {lo!r} > hi = {hi!r}")
        if connectivity not in (6, 26) or isinstance(connectivity, bool):
            raise ValueError(f"connectivity must be 6 or 26, not {connectivity!r}")
        if box is None:
            blo, bhi = (0, 0, 0), tuple(e - 1 for e in ext)
        else:
            try:
                blo, bhi = (tuple(v) for v in box)
            except (TypeError, ValueError):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)), not {box!r}") from None
            if len(blo) != 3 or len(bhi) != 3 or any(isinstance(a, bool) or int(a) != a for a in blo + bhi):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not {box!r}")
            blo, bhi = tuple(int(a) for a in blo), tuple(int(a) for a in bhi)
            if not all(0 <= a <= b < e for a, b, e in zip(blo, bhi, ext)):
                raise ValueError(f"box {box!r} is empty or outside the index extent {tuple(ext)}")
        if isinstance(max_rounds, bool) or int(max_rounds) != max_rounds or not 0 <= int(max_rounds) < 2 ** 32:
            raise ValueError(f"max_rounds must be an integer 0 .. 2^32 - 1, not {max_rounds!r}")
        q.seed[0], q.seed[1], q.seed[2] = (int(a) for a in sd)
        q.lo, q.hi = float(lo32), float(hi32)
        q.connectivity = int(connectivity)
        q.box_lo[0], q.box_lo[1], q.box_lo[2] = blo
        q.box_hi[0], q.box_hi[1], q.box_hi[2] = bhi
        q.max_rounds = int(max_rounds)
        p = self.bind_uniforms()
        res = _abi.VxSegmentResult()
        self._check(self._lib.vx_segment(self._ctx, C.byref(q), C.byref(res)))
        return self._segment_result(res, p)

    def _segment_result(self, res, p, restart: bool = True) -> Segment:
        """the `Segment` of a VxSegmentResult under the uniforms p just bound (segment, segment_edit, set_segment_mask); the
        masked views show the new mask, so accumulation restarts when one is on"""
        if restart and self.segment_view != "off":
            self.restart_rendering()
        g3 = np.asarray(self.volume.grid.transform, dtype=np.float64)[:3, :3]
        d3 = np.asarray(p.density_transform[:], dtype=np.float32).astype(np.float64).reshape(4, 4).T[:3, :3]
        n = int(res.count)
        return Segment(count=n, bbox_lo=tuple(res.bbox_lo[:]), bbox_hi=tuple(res.bbox_hi[:]), d_min=float(res.d_min),
                       d_max=float(res.d_max), d_sum=float(res.d_sum), mean=float(res.d_sum) / n if n else math.nan,
                       rounds=int(res.rounds), converged=bool(res.converged), brick_visits=int(res.brick_visits),
                       volume_grid=n * abs(float(np.linalg.det(g3))), volume_world=n * abs(float(np.linalg.det(d3))))

    SEGMENT_EDIT_OPS = ("dilate", "erode", "open", "close", "fill_holes")   # VxSegmentEditOp, in order

    def segment_edit(self, op: str, steps: int = 1, connectivity: int = 6, band: bool = False) -> Segment:
        """Edits the current segment on the GPU (vx_segment_edit, DESIGN.md section 2 "Segment edits"): "dilate" / "erode" by
        `steps` voxels of the 6- or 26-neighbourhood (outside the volume counts as not set for dilate and as set for erode),
        "open" (erode then dilate), "close" (dilate then erode), or "fill_holes" (the background components, under
        `connectivity`, that touch no face of the volume; steps is ignored).  band=True (dilate only) grows only into voxels
        that pass the predicate of the last segment().  Binds the current uniforms first; returns the `Segment` of the edited
        mask (rounds and brick_visits: the fill's background flood)."""
        if self.volume is None:
            raise VolxelError("segment_edit: no volume (setup_from_grid first)")
        if op not in self.SEGMENT_EDIT_OPS:
            raise ValueError(f"op must be one of {self.SEGMENT_EDIT_OPS}, not {op!r}")
        if connectivity not in (6, 26) or isinstance(connectivity, bool):
            raise ValueError(f"connectivity must be 6 or 26, not {connectivity!r}")
        fill = op == "fill_holes"
        lo = 0 if fill else 1
        hi = 1 if fill else _abi.SEGEDIT_MAX_STEPS
        if isinstance(steps, bool) or not isinstance(steps, (int, np.integer)) or not lo <= int(steps) <= hi:
            raise ValueError(f"steps must be an integer {lo} .. {hi} for {op}, not {steps!r}")
        if not isinstance(band, (bool, np.bool_)):
            raise ValueError(f"band must be a bool, not {band!r}")
        if band and op != "dilate":
            raise ValueError(f"band is for dilate only, not {op}")
        q = _abi.VxSegmentEditParams()
        q.op, q.connectivity, q.steps, q.band = _abi.SEGEDIT_OPS[op], int(connectivity), int(steps), int(bool(band))
        p = self.bind_uniforms()
        res = _abi.VxSegmentResult()
        self._check(self._lib.vx_segment_edit(self._ctx, C.byref(q), C.byref(res)))
        return self._segment_result(res, p)

    def set_segment_mask(self, mask) -> Segment:
        """Installs a (Z, Y, X) bool array over the index extent as the current segment (vx_segment_write_mask, the inverse of
        segment_mask): a saved segmentation, a host-side combination of masks, or an undo.  The predicate of the last
        segment() and the segment view stay.  Binds the current uniforms first; returns the mask's `Segment`."""
        if self.volume is None:
            raise VolxelError("set_segment_mask: no volume (setup_from_grid first)")
        X, Y, Z = (int(e) for e in self.volume.grid.index_extent)
        m = np.asarray(mask)
        if m.dtype != np.bool_:
            raise ValueError(f"mask must be a bool array, not {m.dtype}")
        if m.shape != (Z, Y, X):
            raise ValueError(f"mask shape must be (Z, Y, X) = {(Z, Y, X)} of the index extent, not {m.shape}")
        bits = np.packbits(np.ascontiguousarray(m).ravel(), bitorder="little")
        p = self.bind_uniforms()
        res = _abi.VxSegmentResult()
        self._check(self._lib.vx_segment_write_mask(self._ctx, bits.ctypes.data, bits.size, C.byref(res)))
        return self._segment_result(res, p)

    def segment_edit_stats(self):
        """(launches, edit_ms, stats_ms) of the last segment_edit or set_segment_mask (vx_segment_edit_stats)"""
        n = C.c_uint32()
        ms = (C.c_double * 2)()
        self._check(self._lib.vx_segment_edit_stats(self._ctx, C.byref(n), ms))
        return (n.value,) + tuple(ms)

    def threshold(self, lo: float, hi: float = math.inf, box=None) -> Segment:
        """The whole band as the current segment, without a seed (vx_segment_threshold): every voxel with lo <= d(i) <= hi
        inside `box`; arguments as for segment().  It also becomes the predicate of band dilation.  Returns its `Segment`
        (rounds = brick_visits = 0)."""
        if self.volume is None:
            raise VolxelError("threshold: no volume (setup_from_grid first)")
        ext = [int(e) for e in self.volume.grid.index_extent]
        lo32 = np.float32(lo)
        hi32 = np.float32(np.finfo(np.float32).max) if hi == math.inf else np.float32(hi)
        if not (np.isfinite(lo32) and np.isfinite(hi32)):
            raise ValueError(f"lo and hi must be finite (hi may be inf), not {lo!r}, {hi!r}")
        if lo32 > hi32:
            raise ValueError(f"lo = {lo!r} > hi = {hi!r}")
        if box is None:
            blo, bhi = (0, 0, 0), tuple(e - 1 for e in ext)
        else:
            try:
                blo, bhi = (tuple(v) for v in box)
            except (TypeError, ValueError):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)), not {box!r}") from None
            if len(blo) != 3 or len(bhi) != 3 or any(isinstance(a, bool) or int(a) != a for a in blo + bhi):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not {box!r}")
            blo, bhi = tuple(int(a) for a in blo), tuple(int(a) for a in bhi)
            if not all(0 <= a <= b < e for a, b, e in zip(blo, bhi, ext)):
                raise ValueError(f"box {box!r} is empty or outside the index extent {tuple(ext)}")
        q = _abi.VxSegmentParams()
        q.lo, q.hi = float(lo32), float(hi32)
        q.connectivity = 6
        q.box_lo[0], q.box_lo[1], q.box_lo[2] = blo
        q.box_hi[0], q.box_hi[1], q.box_hi[2] = bhi
        p = self.bind_uniforms()
        res = _abi.VxSegmentResult()
        self._check(self._lib.vx_segment_threshold(self._ctx, C.byref(q), C.byref(res)))
        return self._segment_result(res, p)

    def _islands_call(self, name, op, connectivity, keep=0, min_voxels=0, seed=(0, 0, 0)):
        if self.volume is None:
            raise VolxelError(f"{name}: no volume (setup_from_grid first)")
        if connectivity not in (6, 26) or isinstance(connectivity, bool):
            raise ValueError(f"connectivity must be 6 or 26, not {connectivity!r}")
        q = _abi.VxIslandsParams()
        q.op, q.connectivity, q.keep, q.min_voxels = _abi.ISLANDS_OPS[op], int(connectivity), int(keep), int(min_voxels)
        q.seed[0], q.seed[1], q.seed[2] = (int(a) for a in seed)
        p = self.bind_uniforms()
        res = _abi.VxIslandsResult()
        self._check(self._lib.vx_segment_islands(self._ctx, C.byref(q), C.byref(res)))
        self._island_rows = int(res.kept)
        # (labelling leaves the mask as it was: a masked view does not restart)
        return res, self._segment_result(res.seg, p, restart=op != "label")

    def _island_segment(self, res, seg) -> IslandSegment:
        return IslandSegment(**{f: getattr(seg, f) for f in Segment.__dataclass_fields__}, islands=int(res.islands),
                             kept=int(res.kept), largest=int(res.largest))

    def islands(self, connectivity: int = 6) -> Islands:
        """Labels the islands of the current segment on the GPU (vx_segment_islands, DESIGN.md section 2 "Islands"): its 6- or
        26-connected components, ordered by voxel count descending, ties by the first voxel in C order.  The segment is not
        changed.  Returns an `Islands` (count, sizes, table, labels())."""
        res, seg = self._islands_call("islands", "label", connectivity)
        return Islands(self, res, self.island_table(), seg)

    def island_table(self, first: int = 0, n: int | None = None):
        """rows first .. first + n - 1 (default: all the rest) of the current island table as VxIsland structs (vx_islands_read)"""
        if n is None:
            n = max(getattr(self, "_island_rows", 0) - int(first), 0)
        rows = (_abi.VxIsland * max(int(n), 1))()
        self._check(self._lib.vx_islands_read(self._ctx, int(first), int(n), rows))
        return list(rows[:int(n)])

    def island_labels(self) -> np.ndarray:
        """the dense (Z, Y, X) uint32 label volume of the current island table: 0 outside the segment, k + 1 for island k
        (vx_islands_read_labels)"""
        if self.volume is None:
            raise VolxelError("island_labels: no volume")
        X, Y, Z = (int(e) for e in self.volume.grid.index_extent)
        out = np.empty((Z, Y, X), dtype=np.uint32)
        self._check(self._lib.vx_islands_read_labels(self._ctx, out.ctypes.data, out.size))
        return out

    def keep_largest_islands(self, n: int = 1, connectivity: int = 6) -> IslandSegment:
        """Keeps the n largest islands of the current segment (canonical order; n >= the number of islands keeps all).  Returns
        the `Segment` of the new mask with .islands (before), .kept (after) and .largest."""
        if isinstance(n, bool) or not isinstance(n, (int, np.integer)) or not 1 <= int(n) < 2 ** 64:
            raise ValueError(f"n must be an integer >= 1, not {n!r}")
        return self._island_segment(*self._islands_call("keep_largest_islands", "keep_largest", connectivity, keep=n))

    def remove_small_islands(self, min_voxels: int, connectivity: int = 6) -> IslandSegment:
        """Removes the islands of fewer than min_voxels voxels from the current segment (none left is legal)."""
        if isinstance(min_voxels, bool) or not isinstance(min_voxels, (int, np.integer)) or not 1 <= int(min_voxels) < 2 ** 64:
            raise ValueError(f"min_voxels must be an integer >= 1, not {min_voxels!r}")
        return self._island_segment(*self._islands_call("remove_small_islands", "remove_small", connectivity,
                                                        min_voxels=min_voxels))

    def keep_island_at(self, voxel, connectivity: int = 6) -> IslandSegment:
        """Keeps the island of the current segment that holds `voxel` = (x, y, z); the empty set when the voxel is not in it."""
        if self.volume is None:
            raise VolxelError("keep_island_at: no volume (setup_from_grid first)")
        ext = [int(e) for e in self.volume.grid.index_extent]
        sd = tuple(voxel)
        if len(sd) != 3 or any(isinstance(a, bool) or int(a) != a for a in sd):
            raise ValueError(f"voxel must be three integer voxel indices (x, y, z), not {voxel!r}")
        if not all(0 <= int(a) < e for a, e in zip(sd, ext)):
            raise ValueError(f"voxel {voxel!r} is outside the index extent {tuple(ext)}")
        return self._island_segment(*self._islands_call("keep_island_at", "keep_at", connectivity, seed=sd))

    def islands_stats(self):
        """(launches, local_ms, merge_ms, flatten_ms, table_ms, host_rank_ms, apply_ms, stats_ms) of the last islands call
        (vx_islands_stats); host_rank_ms is the host's wall clock for reading back, ranking and re-uploading the rows"""
        n = C.c_uint32()
        ms = (C.c_double * 7)()
        self._check(self._lib.vx_islands_stats(self._ctx, C.byref(n), ms))
        return (n.value,) + tuple(ms)

    def extract_mesh(self, iso=None, *, segment: bool = False, box=None, space: str = "world", max_vertices: int = 0,
                     max_triangles: int = 0) -> Mesh:
        """The surface of the isosurface d = iso, or (segment=True) of the current segment, as a closed, indexed triangle mesh
        (vx_mesh_extract, DESIGN.md section 2 "Meshes": naive surface nets on the GPU).  Exactly one of iso / segment=True.
        box = ((x0, y0, z0), (x1, y1, z1)), inclusive voxel indices, or None for the whole volume; voxels outside it (and
        outside the volume) count as outside, so the mesh is capped there.  space: "voxel" (voxel i at i, the device's
        coordinates), "grid" (grid.transform * (q + 1/2, 1): mm for DICOM, the space of Segment.volume_grid) or "world" (the
        space of pick()).  max_vertices / max_triangles: refuse a larger mesh (0: 2^32 - 2).  Binds the current uniforms."""
        iso32 = check_extract_args(iso, segment, space, max_vertices, max_triangles)
        if self.volume is None:
            raise VolxelError("extract_mesh: no volume (setup_from_grid first)")
        ext = [int(e) for e in self.volume.grid.index_extent]
        if box is None:
            blo, bhi = (0, 0, 0), tuple(e - 1 for e in ext)
        else:
            try:
                blo, bhi = (tuple(v) for v in box)
            except (TypeError, ValueError):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)), not {box!r}") from None
            if len(blo) != 3 or len(bhi) != 3 or any(isinstance(a, bool) or int(a) != a for a in blo + bhi):
                raise ValueError(f"box must be ((x0, y0, z0), (x1, y1, z1)) of integers, not {box!r}")
            blo, bhi = tuple(int(a) for a in blo), tuple(int(a) for a in bhi)
            if not all(0 <= a <= b < e for a, b, e in zip(blo, bhi, ext)):
                raise ValueError(f"box {box!r} is empty or outside the index extent {tuple(ext)}")
        q = _abi.VxMeshParams()
        q.source = _abi.MESH_SEGMENT if segment else _abi.MESH_DENSITY
        q.iso = 0.0 if segment else float(iso32)
        q.box_lo[0], q.box_lo[1], q.box_lo[2] = blo
        q.box_hi[0], q.box_hi[1], q.box_hi[2] = bhi
        q.max_vertices, q.max_triangles = int(max_vertices), int(max_triangles)
        self.bind_uniforms()
        res = _abi.VxMeshResult()
        self._check(self._lib.vx_mesh_extract(self._ctx, C.byref(q), C.byref(res)))
        self.last_mesh_result = res
        nv, nt = int(res.vertices), int(res.triangles)
        verts = np.empty((nv, 3), dtype=np.float32)
        cells = np.empty((nv, 3), dtype=np.int32)
        tris = np.empty((nt, 3), dtype=np.uint32)
        self._check(self._lib.vx_mesh_read(self._ctx, verts.ctypes.data_as(C.c_void_p), cells.ctypes.data_as(C.c_void_p),
                                           tris.ctypes.data_as(C.c_void_p)))
        mesh = Mesh(verts.astype(np.float64), cells, tris, "voxel")
        if space == "voxel":
            return mesh
        half = np.eye(4)
        half[:3, 3] = 0.5   # voxel i occupies [i, i + 1] in index space
        m = np.asarray(self.volume.grid.transform if space == "grid" else self.volume.combined_transform(), dtype=np.float64)
        return mesh.transformed(m @ half, space)

    def mesh_stats(self):
        """(launches, inside_ms, active_and_scan_ms, emit_ms) of the last extract_mesh (vx_mesh_stats)"""
        n = C.c_uint32()
        ms = (C.c_double * 3)()
        self._check(self._lib.vx_mesh_stats(self._ctx, C.byref(n), ms))
        return (n.value,) + tuple(ms)

    SEGMENT_VIEWS = ("off", "only", "hide")   # VX_SEGVIEW_OFF, _ONLY, _HIDE

    @property
    def segment_view(self) -> str:
        """"off" (the default, and again after setup_from_grid), "only" (the current segment alone) or "hide" (everything but
        it): DVR, Phong, MIP / MinIP renders and the isosurfaces (hence pick) sample a volume whose hidden voxels read 0
        (vx_set_segment_view, DESIGN.md section 2 "Segment views"); slices and segment() keep the unmasked data"""
        v = C.c_int32()
        self._check(self._lib.vx_get_segment_view(self._ctx, C.byref(v)))
        return self.SEGMENT_VIEWS[v.value]

    @segment_view.setter
    def segment_view(self, view: str):
        if view not in self.SEGMENT_VIEWS:
            raise VolxelError(f"segment_view must be one of {self.SEGMENT_VIEWS}, not {view!r}")
        self._check(self._lib.vx_set_segment_view(self._ctx, self.SEGMENT_VIEWS.index(view)))
        self.restart_rendering()

    def segment_mask(self) -> np.ndarray:
        """the current segment as a (Z, Y, X) bool array over the index extent (vx_segment_read_mask)"""
        if self.volume is None:
            raise VolxelError("segment_mask: no volume")
        X, Y, Z = (int(e) for e in self.volume.grid.index_extent)
        bits = np.empty(X * Y * Z // 8, dtype=np.uint8)
        self._check(self._lib.vx_segment_read_mask(self._ctx, bits.ctypes.data, bits.size))
        return np.unpackbits(bits, bitorder="little").astype(bool).reshape(Z, Y, X)

    def slice_mask(self, sp) -> np.ndarray:
        """the current segment on the slice or slab sp (volxel_amd.mpr; reduce, display and window are ignored): an (H, W)
        bool array, True where the nearest voxel of any slab sample is in the segment (vx_slice_segment_mask)"""
        if not isinstance(sp, _abi.VxSliceParams):
            raise TypeError("sp must be a VxSliceParams (volxel_amd.mpr builds them)")
        W, H, N = int(sp.size[0]), int(sp.size[1]), int(sp.slab_samples)
        if not (1 <= W <= _abi.SLICE_MAX_SIZE and 1 <= H <= _abi.SLICE_MAX_SIZE):
            raise ValueError(f"slice size must be 1 .. {_abi.SLICE_MAX_SIZE} per side, not {W} x {H}")
        if not 1 <= N <= _abi.SLICE_MAX_SAMPLES:
            raise ValueError(f"slab_samples must be 1 .. {_abi.SLICE_MAX_SAMPLES}, not {N}")
        for name in ("origin", "du", "dv", "dn"):
            if not np.isfinite(np.asarray(getattr(sp, name)[:], dtype=np.float32)).all():
                raise ValueError(f"slice {name} must be finite")
        out = np.empty((H, W), dtype=np.uint8)
        self._check(self._lib.vx_slice_segment_mask(self._ctx, C.byref(sp), out.ctypes.data))
        return out.astype(bool)

    def segment_stats(self):
        """(rounds, brick_visits, predicate_ms, flood_ms, stats_ms) of the last segment; flood_ms runs from the first round to
        the last, the host's read-backs of the worklist length included"""
        n, v = C.c_uint32(), C.c_uint64()
        ms = (C.c_double * 3)()
        self._check(self._lib.vx_segment_stats(self._ctx, C.byref(n), C.byref(v), ms))
        return (n.value, v.value) + tuple(ms)

    def voxel_index(self, world_point):
        """the voxel (x, y, z) nearest a world point, or None outside the volume: q = density_transform_inv * w - 1/2 in float64
        (the current params, as mpr.oblique maps planes), then floor(q + 1/2) per axis.  A point from pick() lies on the
        interpolated surface, so its nearest voxel can fall just below the threshold: seed a segment with it where the
        structure is thicker than a voxel, or lower lo a little."""
        if self.volume is None:
            raise VolxelError("voxel_index: no volume")
        w = np.asarray(world_point, dtype=np.float64).reshape(-1)
        if w.size != 3 or not np.isfinite(w).all():
            raise ValueError(f"world_point must be three finite numbers, not {world_point!r}")
        # the float32 matrix the uniforms carry now (compute_params, as bind_uniforms sends it), not a copy from an earlier bind
        p = compute_params(self.settings, self.camera, self.volume, self.density_scale, self.width, self.height,
                           self.env_strength, self.shard_rank, self.shard_count, has_environment=self.environment is not None)
        m = [float(v) for v in np.asarray(p.density_transform_inv[:], dtype=np.float32)]   # column major
        # q = m * w - 1/2 in float64, each row summed x, y, z, translation in that order (the JS host's voxelIndex sums alike)
        qv = [m[r] * w[0] + m[4 + r] * w[1] + m[8 + r] * w[2] + m[12 + r] - 0.5 for r in range(3)]
        i = [math.floor(a + 0.5) for a in qv]
        ext = [int(e) for e in self.volume.grid.index_extent]
        if not all(0 <= a < e for a, e in zip(i, ext)):
            return None
        return tuple(int(a) for a in i)

    def probe_gather_rate(self, lines: int, distinct: int | None = None):
        """clocks per 16-byte-per-lane gather instruction per CU (nominal clock) when the 64 lanes form `lines` groups of
        consecutive lanes, each inside one L1-resident line, using `distinct` (default: lines) different lines; and the
        nominal clock in kHz"""
        clk, khz = C.c_double(), C.c_uint32()
        d = int(lines) if distinct is None else int(distinct)
        self._check(self._lib.vx_probe_gather_rate(self._ctx, int(lines), d, C.byref(clk), C.byref(khz)))
        return clk.value, khz.value

    def probe_valu_rate(self):
        """clocks (nominal) per wave64 VALU instruction per SIMD this device sustains, and the nominal clock in kHz"""
        clk, khz = C.c_double(), C.c_uint32()
        self._check(self._lib.vx_probe_valu_rate(self._ctx, C.byref(clk), C.byref(khz)))
        return clk.value, khz.value

    def probe_gather_spread(self, frame_index: int = 0):
        """(q0 gather instructions, wave-wide distinct lines, quad line look-ups) of one DVR frame"""
        out = (C.c_uint64 * 3)()
        self.bind_uniforms()
        self._check(self._lib.vx_probe_gather_spread(self._ctx, int(frame_index), out))
        return int(out[0]), int(out[1]), int(out[2])

    def device_info(self):
        name = C.create_string_buffer(256)
        cus, mem = C.c_uint32(), C.c_uint64()
        self._check(self._lib.vx_device_info(self._ctx, name, 256, C.byref(cus), C.byref(mem)))
        return name.value.decode(), cus.value, mem.value

    # -- multi-GPU load balance: dealing order of the 64x64 tiles (no counterpart in the reference) ----
    def probe_tile_costs(self) -> np.ndarray:
        """cost estimate of every tile of the image for the current volume / TF / uniforms (identical on
        every rank)"""
        from .tiles import tile_counts
        self.bind_uniforms()
        n = tile_counts(self.width, self.height, self.shard_count)[2]
        costs = np.zeros(n, dtype=np.uint32)
        self._check(self._lib.vx_probe_tile_costs(self._ctx, costs.ctypes.data, n))
        return costs

    def set_tile_order(self, perm):
        """perm: position -> tile (a permutation, the same on all ranks) or None for the default dealing;
        restarts the accumulation"""
        if perm is None:
            self._check(self._lib.vx_set_tile_order(self._ctx, None, 0))
        else:
            p = np.ascontiguousarray(perm, dtype=np.uint32)
            self._check(self._lib.vx_set_tile_order(self._ctx, p.ctypes.data, p.size))
        self.tile_order = None if perm is None else np.array(perm, dtype=np.uint32)
        self.restart_rendering()

    def balance_tiles(self):
        """probe the tile costs and deal the tiles so that every shard gets an equal share of the work"""
        from .tiles import balanced_order
        perm = balanced_order(self.probe_tile_costs(), len(self.devices) if self.devices else self.shard_count)
        self.set_tile_order(perm)
        return perm

    # -- zero-copy slab access for the RCCL gather (volxel_amd/dist.py) -----------------
    def slab_info(self):
        n, t = C.c_uint64(), C.c_uint32()
        self._check(self._lib.vx_slab_info(self._ctx, C.byref(n), C.byref(t)))
        return n.value, t.value

    def slab_device_ptr(self) -> int:
        p = C.c_void_p()
        self._check(self._lib.vx_slab_device_ptr(self._ctx, C.byref(p)))
        return p.value

    def detile(self, gathered_dev_ptr: int, image_dev_ptr: int):
        self._check(self._lib.vx_detile(self._ctx, C.c_void_p(gathered_dev_ptr),
                                        C.c_void_p(image_dev_ptr)))
