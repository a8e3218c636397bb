/*
 * volxel_hip.h -- C ABI of libvolxel_hip.so, the MI355X (gfx950) drop-in for the
 * render boundary of Volxel's volxel-3d-viewer.
 *
 * The reference drives its hot path (the per-pixel volume ray loop of
 * volxel-3d-viewer/src/shaders/fragment.frag) through a set of WebGL2 calls issued by
 * volxel-3d-viewer/src/viewer.ts.  Every entry point below replaces one group of those
 * calls; the citation says which.  All paths are relative to the reference repository.
 *
 * Conventions
 *   - plain C, no exceptions, no callbacks; every call returns an int status
 *     (VX_OK == 0) and vx_last_error() returns the message of the last failure, which
 *     the host turns into the `throw new Error(...)` of viewer.ts:797-816;
 *   - one context is used from one thread at a time (the reference is single threaded,
 *     viewer.ts:1160);
 *   - host pointers are read synchronously and may be dropped by the caller on return
 *     (the texImage3D contract of viewer.ts:1106-1142);
 *   - matrices are 16 floats, column major (gl-matrix / math.gl convention);
 *   - framebuffers are RGBA32F, row 0 = bottom row (GL origin, vertex.vert:9).
 */
#ifndef VOLXEL_HIP_H
#define VOLXEL_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define VX_OK 0
#define VX_ERR_INVALID 1      /* bad argument / call order                                */
#define VX_ERR_DEVICE 2       /* HIP runtime failure (message has hipGetErrorString)      */
#define VX_ERR_NO_VOLUME 3    /* render before vx_upload_volume (viewer.ts:1081)          */
#define VX_ERR_NO_DEVICE 4    /* no gfx950 device visible: the product path never falls
                                 back to a CPU implementation                            */

/* render-mode define of the fragment shader (viewer.ts:66-70,771-787, fragment.frag:3). */
enum VxRenderMode {
  VX_MODE_DEFAULT = 0,  /* hierarchical DDA + null collisions   sampling/dda.glsl        */
  VX_MODE_NO_DDA = 1,   /* delta / ratio tracking               sampling/normal.glsl     */
  VX_MODE_RAYMARCH = 2, /* 64-step stochastic march             sampling/raymarch.glsl   */
  VX_MODE_DVR = 3,      /* [build] deterministic front-to-back compositing = E[RAYMARCH],
                           SURVEY.md section 8 row A12 -- the BASELINE.json headline loop */
  VX_MODE_DVR_PHONG = 4, /* [build] DVR + central-difference gradient + Phong (config 4) */
  /* [build] intensity projections ("projections"): the samples of VX_MODE_DVR (ray set-up, jitter
     draws, dvr_step_voxels, dvr_max_steps, clip box, march contract), density d_k = trilinear(q_k) * volume_inv_maj; a ray
     with n >= 1 samples reduces them to m = max_k d_k (MIP) or m = min_k d_k (MinIP) and shows rgba = TF(m) (0 outside
     sample_range) as (r*a, g*a, b*a, 1); a ray that misses or has n = 0 gives (0, 0, 0, 1).  dvr_ert_tau, dvr_gain, the
     Phong terms, bounces, use_env and show_environment have no effect; debug_hits acts as for DVR; the running mean is
     fragment.frag:158's.  dvr_skip_empty = 1: range skipping -- the LDS-window kernel flies over a macro cell whose
     density bound (from the per-brick ranges, widened against rounding) cannot change m: upper bound <= m for MIP, lower
     bound >= m for MinIP.  Exact: the image is bit-identical with skipping on or off.  dvr_shadow_stride must be 0. */
  VX_MODE_MIP = 5,     /* maximum-intensity projection (CT angiography, bone)                                     */
  VX_MODE_MINIP = 6    /* minimum-intensity projection (airways, lung)                                            */
};

/* device layout of the brick grid the trilinear look-ups sample (vx_set_layout) */
enum VxLayout {
  VX_LAYOUT_REFERENCE = 0, /* the three reference textures, linear buffers (common.glsl:35-43) */
  VX_LAYOUT_CELLQUAD = 1,  /* MI355X native: apron bricks of pre-decoded fp32 xy-quads (18 bytes per
                              voxel), two 16-byte gathers per trilinear look-up; the DVR kernel keeps
                              batches of 4 steps in flight per wave                              */
  VX_LAYOUT_BRICKF32 = 2,  /* MI355X native: 8^3 bricks decoded to fp32, 2 KiB contiguous each (4 bytes
                              per voxel); the DVR / Phong kernel stages the window of voxels a wave is
                              marching through into LDS and takes every tap from there           */
  VX_LAYOUT_AUTO = 3,      /* default: each render mode on the layout its kernels are fastest on -- DVR and
                              DVR + Phong on BRICKF32 (built at upload), the path-traced reference modes on
                              CELLQUAD (built the first time such a mode is rendered); volumes beyond the index
                              range of a layout fall back to REFERENCE for the modes concerned       */
  VX_LAYOUT_BRICKU8 = 4    /* MI355X native, opt-in: the 8^3 bricks of BRICKF32 kept as the atlas' 8-bit codes
                              (1 byte per voxel, 512 B per brick) + {min, max - min} per brick; the DVR / Phong
                              kernel decodes them with A4's own fma while it stages a window into LDS -- the same
                              bits as BRICKF32 at a quarter of the memory, a few per cent slower (the march is
                              bound by the vector ALUs, not by HBM).  The path-traced modes sample the
                              reference textures under this layout.                                     */
};

/*
 * The uniform block of fragment.frag / utils.glsl / environment.glsl, one POD.
 * Field-for-field the values viewer.ts:1295-1357 and scene.ts:53-56 bind; the host side
 * (volxel_amd/renderer.py, js/viewer.js) fills it exactly like bindUniforms() does.
 * Every member is 4 bytes wide, no padding.
 */
typedef struct VxParams {
  /* utils.glsl:20-21, set at scene.ts:53-56 */
  float camera_view[16];
  float camera_proj[16];
  /* inverse(camera_view) / inverse(camera_proj): the shader inverts per fragment
     (utils.glsl:24,29,35); hoisted to the host (quirk Q11). */
  float camera_view_inv[16];
  float camera_proj_inv[16];
  /* [build] 0: the reference's perspective ray (utils.glsl:23-40; scene.ts:65-72 is perspective
     only).  1: orthographic -- parallel rays (BASELINE config 1): origin = the unprojected near-plane
     point inverse(view)*inverse(proj)*(ndc.xy,-1,1), direction = normalize(inverse(view)*(0,0,-1,0));
     camera_proj is then a gl-matrix ortho() matrix.                                              */
  int32_t camera_ortho;

  /* fragment.frag:22, viewer.ts:1319-1320 (already clipped by volumeClipMin/Max) */
  float volume_aabb_min[3];
  float volume_aabb_max[3];
  /* fragment.frag:24-30, viewer.ts:1321-1327 */
  float volume_min;
  float volume_maj;
  float volume_inv_maj;
  float volume_albedo[3];
  float volume_phase_g;
  float volume_density_scale;
  /* fragment.frag:34-35, viewer.ts:1329-1331 */
  float density_transform[16];
  float density_transform_inv[16];
  /* fragment.frag:43, viewer.ts:1343 */
  float sample_range[2];

  /* environment.glsl:7-16,  viewer.ts:1303,1338-1340, environment.ts:82-84 */
  float light_dir[3];
  float env_strength;
  int32_t show_environment;
  int32_t use_env; /* 0: directional light (environment.glsl:30-33); 1: the uploaded environment
                      map (environment.glsl:35-79), needs vx_upload_environment first           */
  int32_t bounces;

  /* fragment.frag:44-51, viewer.ts:1351-1356 */
  int32_t res[2]; /* u_res; also the render size (quirk Q2 dropped)                       */
  int32_t debug_hits;

  int32_t render_mode; /* enum VxRenderMode */

  /* [build] parameters of VX_MODE_DVR*; shared verbatim by oracle and kernel            */
  float dvr_step_voxels; /* march step in index-space voxels (BASELINE config: 0.5)      */
  float dvr_ert_tau;     /* early ray termination once optical depth tau >= this
                            (= -ln(eps) for a transmittance threshold eps)               */
  int32_t dvr_jitter;    /* 1: sub-pixel + start jitter from the RNG like the reference
                            (fragment.frag:146, raymarch.glsl:30); 0: pixel centre,
                            start offset 0.5 step                                        */
  int32_t dvr_max_steps; /* samples per ray at most, 0 .. 2^24 (the step index is an fp32 value:
                            t_k = fma(k, dt, t0)); vx_set_params refuses more            */
  int32_t dvr_skip_empty; /* 1: exact empty-space skipping -- samples whose macro cell (16..64
                             voxels) can only see TF-transparent bricks are
                             not evaluated (their alpha is exactly 0) and not counted; for
                             VX_MODE_MIP / VX_MODE_MINIP: range skipping (see VxRenderMode) */
  float dvr_gain[3];     /* albedo * mis * f_p * Le / pdf  (fragment.frag:94-97), host-computed */
  /* Phong terms of VX_MODE_DVR_PHONG */
  float phong_ka, phong_kd, phong_ks, phong_shininess;

  /* image-space sharding: this context renders the tiles
     t with t % shard_count == shard_rank, tile = shard_tile x shard_tile pixels        */
  int32_t shard_rank;
  int32_t shard_count;

  /* [build] shadowed DVR ("light grid"): 0 = off (plain DVR, zero-initialised hosts keep it);
     1, 2 or 4 = stride in voxels of the light grid -- transmittance toward the directional light, built on the device
     and looked up at every contributing DVR sample (w = dT * T_L).  vx_set_params refuses other values, a non-zero
     stride with VX_MODE_DVR_PHONG, and a non-zero stride with VX_MODE_DVR and use_env = 1 (an environment map has no
     single light direction).  The path-traced modes and debug_hits ignore it: they trace real shadows.          */
  int32_t dvr_shadow_stride;
} VxParams;

/* exact work counters of the launches since the last vx_reset_counters */
typedef struct VxCounters {
  uint64_t samples;      /* volume sample evaluations (density lookup + TF + accumulate)  */
  uint64_t rays;         /* primary rays that hit the clipped AABB                        */
  uint64_t pixels;       /* pixels written                                                */
  uint64_t skip_steps;   /* DDA / empty-space steps (not samples).  VX_MODE_MIP / VX_MODE_MINIP: the SAMPLES flown over
                            by range skipping; there samples + skip_steps is exactly the sum of n over the rays */
  uint64_t grad_samples; /* samples that also evaluated the 6-tap gradient (DVR_PHONG)    */
  uint64_t lane_slots;   /* 64 x wave iterations of the DVR march loop (samples / lane_slots
                            = SIMD lane utilisation); 0 for kernels that do not count it   */
  uint64_t launches;     /* render-kernel launches (one launch may cover several frames)   */
  uint64_t frames;       /* accumulation frames rendered                                  */
  double kernel_ms;      /* sum of HIP-event durations of those launches                  */
  double last_kernel_ms; /* duration of the most recent launch                            */
  uint64_t gathers;      /* 16-byte-per-lane gather instructions (global_load_dwordx4 wave
                            instructions) issued by the tuned DVR kernels; 0 for the others  */
  uint64_t lds_reads;    /* LDS tap reads (ds_read wave instructions) of the LDS-tile kernels  */
  double merge_ms;       /* sum of HIP-event durations of the running-mean blend kernels that
                            follow multi-frame launches (fragment.frag:158 applied in order)  */
  uint32_t min_launch_frames; /* smallest / largest number of accumulation frames one launch  */
  uint32_t max_launch_frames; /* actually covered (what ran, not what was requested)           */
  uint64_t tf_samples;   /* samples whose density lay inside the sample range: the ones that fetch a
                            transfer-function entry (common.glsl:78-83) and enter the composite.
                            VX_MODE_MIP / VX_MODE_MINIP: one per ray that has a sample (the TF fetch of m)  */
  uint64_t active_lane_slots; /* of lane_slots, the slots whose lane did work -- counted by the path-traced modes
                            (default / no_dda / raymarch), whose lanes wait for the slowest lane of their wave;
                            0 elsewhere (for the DVR kernels samples / lane_slots is the lane utilisation)  */
  uint64_t merge_launches; /* running-mean blend kernels (merge_results) launched: one per multi-frame launch
                            whose render kernel did not fold the running mean itself                        */
} VxCounters;

typedef struct VxContext VxContext;

#define VX_SHARD_TILE 64 /* pixels per side of one sharding tile */

/* ---- lifecycle: replaces canvas.getContext("webgl2") + program/FBO/texture creation
 *      (viewer.ts:221-414).  device_id = HIP ordinal.  Fails with VX_ERR_NO_DEVICE
 *      when no GPU is present.  */
int vx_create(int device_id, VxContext** out_ctx);

/* ---- device group (no counterpart in the reference): one image rendered on several GPUs from one process.
 * One VxContext per entry of device_ids (a HIP ordinal may repeat), member i renders shard i of n.
 * The returned handle is accepted by the existing entry points; the note "group:" beside each one says what it does
 * with a group.  Fan-out calls run on every member in order (hipSetDevice per member) and stop at the first member
 * that fails; renders are enqueued on every member's stream before anything waits, so distinct devices run
 * concurrently.  The vx_read_* calls gather: one de-tile on the display device (device_ids[0]) reads every member's
 * slab in place -- over xGMI for another device -- after its stream has waited on an event recorded behind each
 * member's last render.  A member's error is reported on the group handle: vx_last_error(group) starts with
 * "member <i> (device <d>): ".  vx_destroy(group) releases every member.
 * Distinct devices: peer access from device_ids[0] to each other device is enabled here; a device it cannot reach
 * fails with VX_ERR_NO_DEVICE (there is no staging-copy fallback).  Repeated ids need no peer access.
 * 1 <= n <= VX_GROUP_MAX, else VX_ERR_INVALID before any device is touched (also for NULL device_ids / out_ctx). */
#define VX_GROUP_MAX 64
int vx_create_group(const int* device_ids, int n, VxContext** out_ctx);

void vx_destroy(VxContext* ctx);
/* message of the last failed call on ctx (ctx may be NULL for vx_create / vx_create_group failures) */
const char* vx_last_error(const VxContext* ctx);

/* run all work of this context on an existing HIP stream (hipStream_t passed as void*);
 * NULL = the context's own stream.  Lets a torch/RCCL host order copies and collectives.
 * group: refused (VX_ERR_INVALID), every member owns its stream. */
int vx_set_stream(VxContext* ctx, void* hip_stream);

/* ---- volume upload: replaces setupFromGrid's four texImage3D groups
 *      (viewer.ts:1106-1142); arguments are field-for-field WasmWorkerMessageDicomReturn
 *      (common.ts:37-55).  `range` and the mips are the LE u16 stream [max,min] per brick
 *      (brick.rs:19-23,357-359).  n_mips must be 3 (brick.rs:13).  group: fan out.  */
int vx_upload_volume(VxContext* ctx,
                     const uint32_t* indirection, const uint32_t indirection_size[3],
                     const uint16_t* range, const uint32_t range_size[3],
                     const uint8_t* atlas, const uint32_t atlas_size[3],
                     int n_mips, const uint16_t* const* mip_data, const uint32_t (*mip_size)[3],
                     const uint32_t index_extent[3]);

/* facts of the last vx_upload_volume on this context: wall seconds (copies + device-side layout build,
 * both inside the call), host bytes moved over PCIe, and whether the atlas could be pinned in place
 * (hipHostRegister) so that the copy engine read it directly -- the "pin/upload volumes to HBM" step.
 * The atlas goes in chunks of whole 8-slice layers and the layout of the brick layers a chunk completes is
 * built behind it on a second stream.  Any out pointer may be NULL.  group: member 0's upload. */
int vx_upload_stats(VxContext* ctx, double* seconds, uint64_t* host_bytes, int* pinned);

/* the same straight from a native brick grid (volxel_brick.h): a C / Rust host that built the grid
 * with vxb_read_dicoms_to_grid or vxb_build_from_u16 uploads it without the copy-out of
 * worker.ts:19-58.  The grid stays owned by the caller (vxb_free afterwards).  group: fan out. */
struct VxBrickGrid;
int vx_upload_brick_grid(VxContext* ctx, const struct VxBrickGrid* grid);

/* select the device layout the trilinear modes sample from (default VX_LAYOUT_AUTO);
 * takes effect at the next vx_upload_volume or immediately if a volume is resident.  group: fan out. */
int vx_set_layout(VxContext* ctx, int layout);

/* ---- transfer function: replaces changeTransferFunc's texImage2D (viewer.ts:1147-1153);
 *      rgba = length x 4 floats, sampled NEAREST + CLAMP_TO_EDGE (viewer.ts:386-389).
 *      group: fan out. */
int vx_upload_transfer(VxContext* ctx, const float* rgba, uint32_t length);

/* ---- environment map: replaces `new Environment(gl, env)` (representation/environment.ts:15-61,
 *      viewer.ts:1076-1077): rgba = width*height*4 floats with row 0 = TOP, exactly the `floats` of
 *      WasmWorkerMessageEnvReturn (the library applies the UNPACK_FLIP_Y_WEBGL of environment.ts:30-32);
 *      builds the 512x512 importance map (shaders/envSetup.frag, 8x8 taps per texel) and its mip
 *      chain on the device.  Needed before VxParams.use_env = 1.  Passing rgba = NULL removes it.  group: fan out. */
int vx_upload_environment(VxContext* ctx, const float* rgba, uint32_t width, uint32_t height);
/* test hook: the importance pyramid, 349525 floats (levels 0..9 of the 512^2 map back to back).  group: member 0. */
int vx_debug_read_importance(VxContext* ctx, float* out);

/* ---- uniforms: replaces bindUniforms + Camera.bindAsUniforms (viewer.ts:1295-1357,
 *      scene.ts:53-56).
 *      group: fan out; member i gets shard_rank = i, shard_count = n.  Params with shard_count != 1 are refused. */
int vx_set_params(VxContext* ctx, const VxParams* params);

/* ---- framebuffers: replaces resizeFramebuffersToCanvas / the two RGBA32F ping-pong
 *      FBOs (viewer.ts:294-324).  Clears the accumulation.  group: fan out. */
int vx_resize(VxContext* ctx, uint32_t width, uint32_t height);

/* ---- one accumulation sample: replaces gl.drawArrays(TRIANGLE_STRIP,0,4) of the
 *      path-tracing program (viewer.ts:1208-1211) including the running-mean blend
 *      out = w*prev + (1-w)*result (fragment.frag:158); frame_index = u_frame_index,
 *      sample_weight = u_sample_weight (viewer.ts:1351,1356).  Asynchronous on the
 *      context's stream.  group: fan out. */
int vx_render_frame(VxContext* ctx, uint32_t frame_index, float sample_weight);

/* The same for `count` consecutive accumulation frames (weights[i] = u_sample_weight of frame
 * first_frame + i), with up to `in_flight` (<= 64) of them rendered by one kernel launch, each into its
 * own result buffer.  Accumulation frames are independent given their index; only the running mean is
 * ordered and it is applied afterwards, in order -- the accumulator is bit-identical to `count` calls of
 * vx_render_frame.  Needs in_flight x (framebuffer + counters) of extra device memory.
 * [build] no reference counterpart: WebGL2 draws are serialised.  group: fan out. */
int vx_render_frames(VxContext* ctx, uint32_t first_frame, uint32_t count, const float* weights, int in_flight);

/* ---- multi-GPU load balance (no counterpart in the reference).  By default tile t of the 64x64 tile grid
 *      (row-major) belongs to shard t % shard_count.  vx_set_tile_order installs another dealing order:
 *      position pos holds tile perm[pos] and belongs to shard pos % shard_count (local index pos /
 *      shard_count), so every shard still owns the same number of tiles.  perm must be a permutation of
 *      0..n_tiles-1 and identical on all ranks; NULL restores the default.  The accumulator is cleared:
 *      restart the accumulation (frame 0) afterwards.  vx_probe_tile_costs fills costs[t] with a cost
 *      estimate of every tile of the image (DVR samples of 64 probe rays per tile, current volume /
 *      transfer function / params) -- the same numbers on every rank, so sorting them gives every rank the
 *      same order without communication.
 *      group: vx_probe_tile_costs runs on member 0 (every member derives the same costs); vx_set_tile_order fans out. */
int vx_probe_tile_costs(VxContext* ctx, uint32_t* costs, uint32_t n_tiles);
int vx_set_tile_order(VxContext* ctx, const uint32_t* perm, uint32_t n_tiles);

/* current framebuffer size (what vx_read_accum / vx_read_display will write).  group: member 0's (all are equal). */
int vx_render_size(VxContext* ctx, uint32_t* width, uint32_t* height);

/* ---- synchronise: replaces gl.finish() (viewer.ts:1214,1289).  group: fan out. */
int vx_finish(VxContext* ctx);

/* ---- readback of the accumulation buffer (what blit.frag samples as u_result),
 *      width*height*4 floats, row 0 = bottom.  Synchronises.
 *      group (also the two display calls): gather every member's shard, then act like one context. */
int vx_read_accum(VxContext* ctx, float* rgba_out);
/* ---- display pass: replaces the blit program (blit.frag:17-35, viewer.ts:1259-1265):
 *      Hable tonemap + gamma, RGBA8, width*height*4 bytes.  Synchronises. */
int vx_read_display(VxContext* ctx, uint8_t* rgba8_out, float exposure, float gamma);
/* ---- the same pass drawn to a canvas of another size, as the viewer does while the low-resolution
 *      preview (resolutionFactor 0.33, viewer.ts:1167-1188) is up: the blit samples u_result with
 *      NEAREST filtering (viewer.ts:310-311), i.e. canvas pixel (x,y) shows render pixel
 *      (floor((x+0.5)*w/out_w), floor((y+0.5)*h/out_h)).  out_w*out_h*4 bytes.  Synchronises. */
int vx_read_display_scaled(VxContext* ctx, uint8_t* rgba8_out, uint32_t out_w, uint32_t out_h,
                           float exposure, float gamma);

/* device-side views for a zero-copy host (torch / RCCL gather): the tile-major slab this
 * shard owns (floats = vx_slab_floats) and a de-tiling pass from a gathered set of slabs.
 * group: all three refused (VX_ERR_INVALID): a group has no single slab. */
int vx_slab_info(VxContext* ctx, uint64_t* slab_floats, uint32_t* tiles_per_shard);
int vx_slab_device_ptr(VxContext* ctx, void** dev_ptr);
/* gathered = shard_count slabs back to back (device pointer); writes row-major W*H*4 floats
 * to image_out (device pointer). */
int vx_detile(VxContext* ctx, const void* gathered_dev, void* image_out_dev);

/* ---- counters: the benchmark harness of viewer.ts:1213-1252 measures wall time around
 *      gl.finish(); here the kernel is bracketed by HIP events on its own stream.
 *      group: vx_reset_counters fans out.  vx_get_counters combines the members': the work counters samples, rays,
 *      pixels, skip_steps, grad_samples, tf_samples, lane_slots, active_lane_slots, gathers, lds_reads, launches and
 *      merge_launches are summed; frames, min_launch_frames and max_launch_frames are member 0's (every member renders
 *      the same frames); kernel_ms, last_kernel_ms and merge_ms are the maximum over the members (the slowest device
 *      bounds the wall time). */
int vx_get_counters(VxContext* ctx, VxCounters* out);
int vx_reset_counters(VxContext* ctx);

/* library / device facts for logs (viewer.ts:225-242 device record).  group: member 0 (the display device).
 * The test and measurement hooks below (vx_debug_*, vx_probe_*), the slices (vx_slice, vx_slice_stats) the isosurfaces
 * (vx_isosurface, vx_iso_stats) and the segments (vx_segment and its siblings) also run on member 0 of a group. */
int vx_device_info(VxContext* ctx, char* name_out, uint32_t name_cap, uint32_t* cu_count,
                   uint64_t* hbm_bytes);
const char* vx_version(void);

/* test hook: the integer RNG of shaders/random.glsl evaluated ON THE DEVICE (rows A1/A2), one thread per
 * output word.  op 0: out[i] = tea(a[i], b[i], 32) (random.glsl:41-51); op 1: out[i] = wangHash(a[i]) (:59-66);
 * op 2: out[0..n) = the first n xoshiro128pp_next words of seedXoshiro(a[0]) (:69-94, quirk Q1);
 * op 3: the same stream as rng() floats, bit patterns (:103-106);
 * op 4: out[i] = how many of the 256 draws r = (256 * (a[0] + i) + j) / 2^24, j = 0..255, give a free-flight logarithm
 * (the library's -log(1 - r), normal.glsl:13,28 / dda.glsl:28,58 / raymarch.glsl:26) that differs in any bit from
 * -logf(1 - r): a[0] = 0, n = 65536 covers every value rng() can return.  a / b / out are host pointers.  */
int vx_debug_rng(VxContext* ctx, int op, const uint32_t* a, const uint32_t* b, uint32_t n, uint32_t* out);

/* measurement hook (no reference counterpart): what the vector L1 of this device sustains for the
 * gather shape of the cellquad DVR march -- wave instructions of 16 bytes per lane whose 64 lanes form `lines`
 * groups of consecutive lanes, each group inside one L1-resident 128-byte line, the groups using `distinct`
 * (<= lines) different lines in turn; nothing else in the loop, 20 waves per CU, 8 gathers in flight per wave.
 * Returns the cost in clocks per gather instruction per CU at the device's nominal clock (clock_khz_out).
 * bench.py calls it for the roofline.l1 block with lines = the march's line look-ups per gather over its
 * 4-lane groups and distinct = its distinct lines per gather over the whole wave. */
int vx_probe_gather_rate(VxContext* ctx, uint32_t lines, uint32_t distinct, double* clk_per_gather_out,
                         uint32_t* clock_khz_out);
/* measurement hook: what the vector ALUs of this device sustain: clocks (nominal clock) per wave64 VALU instruction per
 * SIMD, from independent v_fma_f32 chains at 8 waves per SIMD.  bench.py prices the instruction count of the LDS-window
 * DVR kernel with it (roofline.issue). */
int vx_probe_valu_rate(VxContext* ctx, double* clk_per_instruction_out, uint32_t* clock_khz_out);
/* measurement hook: re-march frame `frame_index` with the current volume / params and count, per gather
 * instruction of the tuned cellquad DVR kernel, the distinct 128-byte lines its active lanes address
 * (whole wave) and the line look-ups of its 16 groups of 4 consecutive lanes (what the L1 tag pipe sees).
 * Nothing is written to the accumulator.  out3 = {gather instructions, distinct lines, quad look-ups}. */
int vx_probe_gather_spread(VxContext* ctx, uint32_t frame_index, uint64_t out3[3]);

/* ---- shadowed DVR (VxParams.dvr_shadow_stride != 0, no reference counterpart): the light grid is rebuilt lazily before
 *      a shadowed DVR launch whenever one of its inputs differs bitwise from the last build (volume or TF upload, light_dir,
 *      density_transform_inv, the clip box, volume_maj / inv_maj / density_scale, sample_range, dvr_step_voxels,
 *      dvr_ert_tau, dvr_max_steps, the stride); a camera move does not rebuild.
 * vx_shadow_stats: light-grid builds since vx_create, light-march samples of the last build and its HIP-event time
 * (synchronises).  Any out pointer may be NULL.  group: member 0 (every member builds its own grid, replicated like the volume). */
int vx_shadow_stats(VxContext* ctx, uint64_t* builds, uint64_t* light_samples, double* last_build_ms);
/* test hook: the last light grid built, dims_out[0] * dims_out[1] * dims_out[2] floats, x fastest (node (i, j, k) at
 * ((k * dims[1]) + j) * dims[0] + i); out = NULL queries the dimensions only.  VX_ERR_INVALID before the first build.
 * Synchronises.  group: member 0. */
int vx_debug_read_shadow_grid(VxContext* ctx, float* out, uint32_t dims_out[3]);

/* ---- slices: multiplanar reformation and thick slabs (no reference counterpart; DESIGN.md section 2 "Slices").
 * A slice is a W x H grid of pixels on a plane, each with N slab samples along dn.  Positions are in the cell frame of the
 * march contract (q = index position - 1/2: the centre of voxel i is at q = i).  Per axis a,
 *   q_a = fma(s, dn_a, fma(y, dv_a, fma(x, du_a, origin_a)))     pixel (x, y), sample s = 0 .. N-1 (exact fp32 integers),
 * d_s = trilinear(q) * volume_inv_maj (A5 on any layout, taps outside the volume read 0, volume_density_scale and
 * volume_inv_maj of the last vx_set_params; the clip box does not apply).  The reduction gives one value per pixel. */
enum VxSliceReduce {
  VX_SLICE_MEAN = 0, /* acc = d_0, acc = acc + d_s for s = 1 .. N-1 in order (fp32 adds), value = acc / N (IEEE)  */
  VX_SLICE_MAX = 1,  /* fmaxf over the d_s: a thick-slab MIP                                                      */
  VX_SLICE_MIN = 2   /* fminf over the d_s: a thick-slab MinIP                                                     */
};
/* the optional RGBA8 display of the values (alpha 255; fp32 operations, no contraction); a byte is
 * (uint8_t)(c * 255 + 0.5) of c clamped to [0, 1] (gl_clamp) */
enum VxSliceDisplay {
  VX_SLICE_NONE = 0, /* no display output                                                                          */
  VX_SLICE_GREY = 1, /* c = (value - window[0]) / (window[1] - window[0]) in r, g and b                            */
  VX_SLICE_TF = 2    /* rgba = TF(value) by DVR's rule (NEAREST bin, 0 outside sample_range), shown (r*a, g*a, b*a) */
};
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxSliceParams {
  float origin[3], du[3], dv[3], dn[3]; /* cell frame, see above                                  */
  uint32_t size[2];                      /* W, H: 1 .. 16384 each                                  */
  uint32_t slab_samples;                 /* N: 1 .. 4096                                           */
  int32_t reduce;                        /* enum VxSliceReduce                                     */
  int32_t display;                       /* enum VxSliceDisplay                                    */
  float window[2];                       /* VX_SLICE_GREY: the values shown black and white        */
} VxSliceParams;
/* One slice on the context's stream, behind every render already queued; synchronises.  values_out: W*H floats, row-major,
 * row 0 = y = 0 (the accumulator's GL convention); rgba8_out: W*H*4 bytes, with a display other than VX_SLICE_NONE only.
 * Either may be NULL; with both NULL only the kernel runs (timing).  The accumulator, the frame state and VxCounters are not
 * touched.  The output buffers (W*H*8 bytes) stay with the context and grow with the largest slice.
 * VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the field, before vx_set_params, for NULL sp, a size, N, reduce
 * or display out of range, a non-finite vector component, a window with window[1] <= window[0] (or not finite) under
 * VX_SLICE_GREY, VX_SLICE_TF without a transfer function, and rgba8_out with VX_SLICE_NONE.
 * group: member 0 (the display device), like the probes. */
int vx_slice(VxContext* ctx, const VxSliceParams* sp, float* values_out, uint8_t* rgba8_out);
/* the last slice: its samples (W*H*N) and the HIP-event time of its kernel; both 0 before the first slice.  Any out pointer
 * may be NULL.  group: member 0. */
int vx_slice_stats(VxContext* ctx, uint64_t* samples, double* last_kernel_ms);

/* ---- isosurfaces: the first hit of a density threshold and per-pixel picking (no reference counterpart; DESIGN.md section 2
 * "Isosurfaces").  Rays and samples are DVR's, from the last vx_set_params (camera, ortho flag, clip box,
 * density_transform_inv, dvr_step_voxels, dvr_max_steps, volume_density_scale, volume_inv_maj), always with the pixel-centre
 * ray and start offset 1/2: dvr_jitter, the shard fields, render_mode and debug_hits have no effect.  Sample k of a ray's n sits
 * at q_k = fma(k, dq, q0) (the march contract) and has d_k = trilinear(q_k) * volume_inv_maj.
 *   hit:     the first k < n with d_k >= iso.  k = 0 is a cap (the ray enters the clip box inside the surface): s* = 0.  Otherwise
 *            `refine` bisection steps on the fp32 sample parameter: lo = k - 1, hi = k; mid = 0.5f * (lo + hi), d at
 *            fma(mid, dq, q0); d >= iso ? hi = mid : lo = mid; s* = hi.  n = 0, or no d_k >= iso: a miss.
 *   hit_out: (w_x, w_y, w_z, t), t = fma(s*, dt, t0) the world ray parameter (>= 0) and w = fma(t, d, o) per axis;
 *            a miss is (0, 0, 0, -1).
 *   rgba_out: Blinn-Phong on color with alpha 1, n = -g/|g| from Phong's central difference at q(s*) in its own cell frame
 *            scaled by the diagonal of density_transform_inv (Frame::dvr<PHONG>); a cap or |g|^2 <= 1e-12 takes n = -ray
 *            direction.  c = color * fma(kd, max(0, n.l), ka) + ks * max(0, n.h)^shininess, l = -light_dir, h as Phong's.
 *            A miss is (0, 0, 0, 0).
 * Hit flags, k, s*, t, w and the counters are exact on every layout, with skipping on or off; the normal and the colour use the
 * hardware rsq / log2 / exp2 as Phong does (tolerance 1e-5).  skip = 1: a sample whose macro cell has an upper density bound
 * (the intensity projections' table) below iso cannot be a hit; it is passed over, counted in `skipped`, not in `samples`. */
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxIsoParams {
  float iso;               /* threshold on d = trilinear(q) * volume_inv_maj, the value DVR hands to the TF  */
  float color[3];          /* surface albedo                                                                 */
  float ka, kd, ks, shininess;
  uint32_t refine;         /* bisection steps, 0 .. 16                                                       */
  int32_t skip;            /* 0 / 1: range skipping                                                          */
  uint32_t window[4];      /* x0, y0, x1, y1 of the render size, x0 <= x < x1; all zero = the whole image    */
} VxIsoParams;
/* One isosurface image of the window on the context's stream, behind every render already queued; synchronises.  rgba_out and
 * hit_out: 4 floats per window pixel, row-major, row 0 = y0; either may be NULL.  The accumulator, the frame state, VxCounters,
 * the light grid and VxParams are not touched; the output buffers (8 floats per window pixel) stay with the context and grow
 * with the largest window.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the field, before vx_set_params, for NULL
 * ip, a non-finite iso, color or Phong term, shininess < 0, refine > 16, skip not 0 / 1, an empty window or one outside the
 * render size, and params set for another mode that fail DVR's march checks (dvr_step_voxels > 0, dvr_max_steps in [0, 2^24]).
 * group: member 0 (the display device), like the slices. */
int vx_isosurface(VxContext* ctx, const VxIsoParams* ip, float* rgba_out, float* hit_out);
/* the last isosurface: rays that hit the clip box, hits, march samples evaluated, bisection samples (refine x hits that are
 * not caps), samples passed over by range skipping, and the HIP-event time of its kernel; all 0 before the first call.  Per ray
 * samples + skipped = k + 1 for a hit, n for a miss.  Any out pointer may be NULL.  group: member 0. */
int vx_iso_stats(VxContext* ctx, uint64_t* rays, uint64_t* hits, uint64_t* samples, uint64_t* refine_samples,
                 uint64_t* skipped, double* last_kernel_ms);

/* ---- segmentation: seeded region growing (no reference counterpart; DESIGN.md section 2 "Segmentation").  Voxel i = (x, y, z)
 * of index_extent has density d(i) = (volume_density_scale * v(i)) * volume_inv_maj (two fp32 products, the last
 * vx_set_params), bit for bit the trilinear density at q = i.  P(i) = lo <= d(i) <= hi and box_lo <= i <= box_hi per axis (the
 * clip box does not apply).  The segment is the connected component of P holding the seed, 6- (faces) or 26-connected (faces,
 * edges, corners); empty when P(seed) is false.  It is unique: the mask does not depend on layout, scheduling or launch shape. */
/* box_hi[a] = VX_SEGMENT_BOX_END: the box reaches the far face of index_extent on axis a (box_lo 0 and box_hi all END: the whole
 * volume).  Every other value is an inclusive voxel index. */
#define VX_SEGMENT_BOX_END 0xffffffffu
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxSegmentParams {
  uint32_t seed[3];        /* voxel index, inside index_extent                                                    */
  float lo, hi;            /* finite, lo <= hi, both bounds inclusive                                             */
  int32_t connectivity;    /* 6 or 26                                                                              */
  uint32_t box_lo[3];      /* inclusive voxel box inside index_extent, box_lo <= box_hi                           */
  uint32_t box_hi[3];      /* or VX_SEGMENT_BOX_END per axis: to the far face                                      */
  uint32_t max_rounds;     /* cap on flood rounds; 0 = the number of voxels (capped at 2^32 - 2), which bounds any component */
} VxSegmentParams;
/* count, bbox (inclusive; all 0 for an empty segment), min / max of d (0 when empty) and the float64 sum of d over the segment:
 * exact and identical from run to run (the sum adds each brick in a fixed voxel order, then the bricks in a fixed tree).
 * rounds (flood launches with a non-empty worklist) and brick_visits may vary from run to run.  converged = 0: max_rounds
 * ended the flood first and the mask is a connected subset of the segment. */
typedef struct VxSegmentResult {
  uint64_t count;
  uint32_t bbox_lo[3], bbox_hi[3];
  float d_min, d_max;
  double d_sum;
  uint32_t rounds, converged;
  uint64_t brick_visits;
} VxSegmentResult;
/* Grows the segment of sp on the context's stream behind every queued render and synchronises; it replaces the context's one
 * segment.  out may be NULL.  The accumulator, the frame state, VxCounters, the light grid, the bound tables and VxParams are not
 * touched.  Reads the layout resident at the call (all layouts give the same bits).  Its buffers (2 x 64 B, 8 B and 4 x 4 B per
 * brick) are allocated on first use and freed with the volume.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the
 * field, before vx_set_params, for NULL sp, a seed outside index_extent, a non-finite lo / hi or lo > hi, connectivity not 6 or
 * 26, and a box that is empty or outside the volume.  group: member 0, like the slices and the isosurfaces. */
int vx_segment(VxContext* ctx, const VxSegmentParams* sp, VxSegmentResult* out);
/* the current segment as one bit per voxel of (z, y, x) in C order, LSB first (np.packbits(mask.ravel(), bitorder="little")):
 * nbytes must be X * Y * Z / 8 of index_extent.  VX_ERR_INVALID with no current segment (none yet, or a volume uploaded since) */
int vx_segment_read_mask(VxContext* ctx, uint8_t* bits, uint64_t nbytes);
/* the segment on a slice: out[y * W + x] = 1 when for any slab sample s the nearest voxel floor(q + 0.5f) per axis (q as in
 * vx_slice: the fma chain and its +-2^24 clamp) is in the volume and in the segment, else 0.  reduce, display and window are
 * ignored; vx_slice's checks on size, slab_samples and finite vectors apply.  VX_ERR_INVALID with no current segment. */
int vx_slice_segment_mask(VxContext* ctx, const VxSliceParams* sp, uint8_t* out);
/* the last segment: flood rounds, brick visits and the HIP-event times of its predicate pass, its flood (from the first round
 * to the last, host read-backs of the worklist length included) and its statistics, kernel_ms[0 .. 2]; all 0 before the first
 * call.  Any pointer may be NULL.  group: member 0. */
int vx_segment_stats(VxContext* ctx, uint32_t* rounds, uint64_t* brick_visits, double* kernel_ms);

/* ---- segment edits (DESIGN.md section 2 "Segment edits"): morphology on the current segment M, a set of voxels of index_extent
 * (padding voxels included).  N_c(i) is voxel i with its 6 face neighbours or its 26 face, edge and corner neighbours.
 *   DILATE      D(M) = { i in the volume : N_c(i) meets M }; voxels outside the volume count as NOT set.  steps applies D n times.
 *               band = 1: D_P(M) = M | (D(M) & P) per step, P the predicate words of the last vx_segment on this volume
 *               ("grow, but only into voxels that pass the threshold"); voxels of M outside P stay.
 *   ERODE       E(M) = ~D(~M), the complement taken inside the volume: voxels outside the volume count as SET, so a structure
 *               cut by the edge of the scan does not erode from outside and the whole volume erodes to itself.
 *   OPEN        D^n(E^n(M));  CLOSE  E^n(D^n(M)), each half with its own border rule: closing is extensive, opening
 *               anti-extensive, both idempotent, also at the faces of the volume.
 *   FILL_HOLES  M | H, H the c-connected components of ~M (inside the volume) that hold no voxel on any of the six faces of
 *               index_extent; connectivity is that of the BACKGROUND.  steps must be 0 or 1 and is ignored.
 * Every result is a unique set: it does not depend on layout, launch shape or scheduling.  An empty M is legal. */
typedef enum VxSegmentEditOp {
  VX_SEGEDIT_DILATE = 0,
  VX_SEGEDIT_ERODE = 1,
  VX_SEGEDIT_OPEN = 2,
  VX_SEGEDIT_CLOSE = 3,
  VX_SEGEDIT_FILL_HOLES = 4
} VxSegmentEditOp;
#define VX_SEGEDIT_MAX_STEPS 1024u
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxSegmentEditParams {
  int32_t op;              /* VxSegmentEditOp                                                                      */
  int32_t connectivity;    /* 6 or 26                                                                              */
  uint32_t steps;          /* 1 .. VX_SEGEDIT_MAX_STEPS; 0 or 1 for FILL_HOLES                                      */
  int32_t band;            /* 0, or 1 with DILATE: only into the predicate of the last vx_segment                  */
} VxSegmentEditParams;
/* Edits the current segment in place, on the context's stream behind every queued render, and synchronises.  out (may be NULL)
 * holds the statistics of the new mask: count, bbox, min / max and the float64 sum as vx_segment computes them (the scale and
 * inv_maj of the last vx_set_params), all 0 when empty; rounds and brick_visits are those of FILL_HOLES' background flood and 0
 * for the other ops; converged = 1.  The accumulator, the frame state, VxCounters, the light grid, the bound tables, VxParams,
 * the segment view and what vx_segment_stats reports are not touched; with a view on, the next covered call reads the edited
 * mask.  Two scratch masks (64 B per brick each: 1 bit per voxel) and 4 B per brick are allocated by the first edit and freed
 * with the volume.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the field, before vx_set_params, for NULL params,
 * an op outside the enum, connectivity not 6 or 26, steps out of range, band not 0 or 1, band = 1 with another op or with no
 * vx_segment on this volume, and with no current segment.  A refused call changes nothing.  group: member 0. */
int vx_segment_edit(VxContext* ctx, const VxSegmentEditParams* params, VxSegmentResult* out);
/* The inverse of vx_segment_read_mask: installs bits (one bit per voxel of (z, y, x) in C order, LSB first, nbytes = X * Y * Z / 8)
 * as the current segment, creating one where there was none, and computes its statistics into out (may be NULL; rounds and
 * brick_visits 0, converged 1).  The predicate words of the last vx_segment and the segment view stay.  Stream, group and
 * untouched state as vx_segment_edit.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID before vx_set_params, for NULL bits
 * and a wrong nbytes. */
int vx_segment_write_mask(VxContext* ctx, const uint8_t* bits, uint64_t nbytes, VxSegmentResult* out);
/* the last vx_segment_edit or vx_segment_write_mask: kernels launched by the edit itself, and the HIP-event times of the edit
 * (FILL_HOLES: host read-backs of the worklist length included) and of the statistics, kernel_ms[0 .. 1]; all 0 before the
 * first call.  Any pointer may be NULL.  group: member 0. */
int vx_segment_edit_stats(VxContext* ctx, uint32_t* launches, double* kernel_ms);

/* ---- islands (DESIGN.md section 2 "Islands"): the c-connected components (c = 6 or 26) of the current segment M inside the
 * volume.  Island I has count(I) voxels, anchor(I) = its first voxel in C order over (z, y, x) and an inclusive bbox.  The
 * canonical order is by count descending, ties by the C-order index of the anchor ascending; island k (0-based) of that order
 * has label k + 1, the background label 0.  All of it is a function of M and c alone: not of layout, launch shape or run. */
/* The whole band as the current segment, without a seed: M = { i : P(i) } (lo, hi and the box as for vx_segment; seed,
 * connectivity and max_rounds are ignored).  The band also becomes the predicate of band dilation, as vx_segment leaves it.
 * out (may be NULL): the statistics as vx_segment computes them, rounds = brick_visits = 0, converged = 1; vx_segment_stats keeps
 * reporting the last vx_segment.  Stream, group, untouched state and refusals (other than the seed's and the connectivity's) as
 * vx_segment.  No new kernel: seg_predicate and seg_stats behind an entry point of their own. */
int vx_segment_threshold(VxContext* ctx, const VxSegmentParams* sp, VxSegmentResult* out);
typedef enum VxIslandsOp {
  VX_ISLANDS_LABEL = 0,         /* changes nothing: labels M and fills the table                                    */
  VX_ISLANDS_KEEP_LARGEST = 1,  /* keeps islands 0 .. keep - 1 of the canonical order (keep >= islands: all)        */
  VX_ISLANDS_REMOVE_SMALL = 2,  /* keeps the islands with count >= min_voxels (none left is legal)                  */
  VX_ISLANDS_KEEP_AT = 3        /* keeps the island that holds voxel seed; the empty set when seed is not in M      */
} VxIslandsOp;
/* every member is 4 or 8 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxIslandsParams {
  int32_t op;              /* VxIslandsOp                                                                          */
  int32_t connectivity;    /* 6 or 26                                                                              */
  uint64_t keep;           /* KEEP_LARGEST: >= 1; ignored by the other ops                                         */
  uint64_t min_voxels;     /* REMOVE_SMALL: >= 1; ignored by the other ops                                         */
  uint32_t seed[3];        /* KEEP_AT: a voxel inside index_extent; ignored by the other ops                       */
  uint32_t reserved;       /* 0                                                                                    */
} VxIslandsParams;
/* islands: the islands of M BEFORE the op; kept: after it; largest: the count of island 0 before the op (0 for an empty M);
 * seg: the statistics of the mask AFTER the op, as vx_segment_edit reports them (rounds = brick_visits = 0, converged = 1) */
typedef struct VxIslandsResult {
  uint64_t islands, kept, largest;
  VxSegmentResult seg;
} VxIslandsResult;
/* one row of the table: x, y, z order in anchor and bbox */
typedef struct VxIsland {
  uint64_t count;
  uint32_t anchor[3];
  uint32_t bbox_lo[3], bbox_hi[3];
  uint32_t label;          /* its place in the canonical order + 1 */
} VxIsland;
/* Labels the current segment and applies op, on the context's stream behind every queued render, and synchronises.  After a
 * modifying op the table and the labels describe the NEW mask (a filter of the old table: the kept islands keep their order).
 * The number of kernel launches is a function of the op alone, never of the mask: a union-find over the brick words, not a flood
 * (vx_islands.hpp).  Labels are 4 B per voxel, with 8 B per brick, allocated by the first call and freed with the volume; the table
 * (40 + 4 B per island) grows to the largest count met.  The accumulator, the frame state, VxCounters, the light grid, the bound
 * tables, the mesh, VxParams, the segment view and what vx_segment_stats reports are not touched; with a view on, the next covered
 * call reads the new mask.  An empty M is legal (0 islands).  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the
 * field and changing nothing, before vx_set_params, for NULL params, no current segment, an op outside the enum, connectivity not
 * 6 or 26, keep = 0 (KEEP_LARGEST), min_voxels = 0 (REMOVE_SMALL), a KEEP_AT seed outside index_extent and a volume of 2^31
 * voxels or more.  out may be NULL.  group: member 0. */
int vx_segment_islands(VxContext* ctx, const VxIslandsParams* params, VxIslandsResult* out);
/* rows first .. first + n - 1 of the table in canonical order.  VX_ERR_INVALID with no current table (none yet; an upload,
 * vx_segment, vx_segment_threshold, vx_segment_edit and vx_segment_write_mask drop it), for first + n beyond the number of
 * islands and for NULL out with n > 0. */
int vx_islands_read(VxContext* ctx, uint64_t first, uint64_t n, VxIsland* out);
/* the dense label volume, (Z, Y, X) in C order: nvoxels must be X * Y * Z of index_extent.  VX_ERR_INVALID with no current table,
 * for NULL labels and a wrong nvoxels.  Its device buffer (4 B per voxel) is allocated by the first read. */
int vx_islands_read_labels(VxContext* ctx, uint32_t* labels, uint64_t nvoxels);
/* the last vx_segment_islands: kernels launched, and kernel_ms[0 .. 6] = the HIP-event times of the in-brick labelling, the
 * merge across bricks, the flattening with the scan of the root counts, the table, the HOST's ranking of the rows (wall clock:
 * the read-back of the rows, the sort and the upload of the labels), the apply pass (0 for LABEL) and the statistics; all 0 before
 * the first call.  Any pointer may be NULL.  group: member 0. */
int vx_islands_stats(VxContext* ctx, uint32_t* launches, double* kernel_ms);

/* ---- distances and margins (DESIGN.md section 2 "Distances and margins"): the squared Euclidean distance transform of the
 * current segment M under an anisotropic voxel spacing s = (s_x, s_y, s_z), and the margins in physical units built on it.
 * Voxels are those of index_extent, padding included.  The source set S is M (side OUTSIDE) or the complement of M inside the
 * volume (side INSIDE); voxels outside the volume are never candidates -- the border rules of DILATE and ERODE.
 *   term     t_a(n) = fl32(p * p), p = fl32(fl32(n) * s_a), for an offset of n voxels on axis a: fp32, no contraction
 *   D2(i)    min over j in S of fl32(fl32(t_x(|dx|) + t_y(|dy|)) + t_z(|dz|)); +inf when S is empty.  Rounding is monotone, so
 *            the minimum separates exactly into an x, a y and a z pass, each a plain minimum over the candidates of a line.
 *   cap      R2 = fl32(r * r) of max_distance / radius r; every voxel with D2 > R2 reports +inf.
 *   GROW     { i : D2_M(i) <= R2 };  band = 1: M | (GROW(M) & P), P the predicate words of the last vx_segment / _threshold
 *   SHRINK   { i in M : D2_complement(i) > R2 }: the whole volume shrinks to itself, the empty set grows to itself
 *   CLOSE    SHRINK(GROW(M));  OPEN  GROW(SHRINK(M))
 * The device holds D2 and never takes a square root: a host takes it of what it reads.  Every result is a unique function of
 * M, s and r: it does not depend on layout, launch shape or scheduling, and two calls give the same bytes. */
typedef enum VxDistanceSide {
  VX_DISTANCE_OUTSIDE = 0,   /* S = M: how far every voxel is from the segment (0 inside it)                          */
  VX_DISTANCE_INSIDE = 1     /* S = the complement: how far every voxel of the segment is from leaving it (0 outside) */
} VxDistanceSide;
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxDistanceParams {
  float spacing[3];        /* s_x, s_y, s_z: finite, > 0 (mm for DICOM: the column norms of grid.transform)             */
  float max_distance;      /* the cap r, > 0, in the units of spacing; +inf: none                                      */
  int32_t side;            /* VxDistanceSide                                                                           */
} VxDistanceParams;
/* finite: the voxels with D2 <= R2 (those of S included).  max_d2: the largest D2 <= R2 over the voxels NOT in S, and argmax
 * (x, y, z) the first voxel in C order over (z, y, x) that attains it; 0 and (0, 0, 0) when there is none.  With side INSIDE
 * sqrt(max_d2) is the radius of the largest ball of voxel centres that fits inside the segment, centred at argmax.
 * every member is 4 or 8 bytes wide, no padding */
typedef struct VxDistanceResult {
  uint64_t finite;
  float max_d2;
  uint32_t argmax[3];
} VxDistanceResult;
/* Computes the field of the current segment on the context's stream behind every queued render and synchronises.  out may be
 * NULL.  The segment, its predicate, the island table, the mesh, the accumulator, the frame state, VxCounters, the light grid,
 * the bound tables, VxParams, the segment view and what the other *_stats calls report are not touched.  The field (4 B per
 * voxel, one field: the y and z passes run in place) and 24 KiB of partial statistics are allocated by the first call and freed
 * with the volume.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the field and changing nothing, before
 * vx_set_params, for NULL params, no current segment, a spacing component that is not finite or <= 0, a max_distance that is
 * NaN or <= 0, an unknown side, and a volume with more than 16384 voxels along y or z (a line the passes cannot hold in LDS).
 * group: member 0. */
int vx_segment_distance(VxContext* ctx, const VxDistanceParams* params, VxDistanceResult* out);
/* the field of the last vx_segment_distance: D2 per voxel, dense (Z, Y, X) in C order, +inf beyond the cap; nvoxels must be
 * X * Y * Z of index_extent.  VX_ERR_INVALID with no current field (none yet; an upload and every call that changes or replaces
 * the segment -- vx_segment, _threshold, _edit, _write_mask, _margin and a modifying vx_segment_islands -- drop it), for NULL d2
 * and a wrong nvoxels. */
int vx_distance_read(VxContext* ctx, float* d2, uint64_t nvoxels);
typedef enum VxMarginOp {
  VX_MARGIN_GROW = 0,
  VX_MARGIN_SHRINK = 1,
  VX_MARGIN_OPEN = 2,
  VX_MARGIN_CLOSE = 3
} VxMarginOp;
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxMarginParams {
  int32_t op;              /* VxMarginOp                                                                               */
  float radius;            /* r: finite, > 0, in the units of spacing                                                  */
  float spacing[3];        /* as VxDistanceParams                                                                      */
  int32_t band;            /* 0, or 1 with GROW: only into the predicate of the last vx_segment / vx_segment_threshold  */
} VxMarginParams;
/* Edits the current segment in place by a margin in physical units, on the context's stream behind every queued render, and
 * synchronises: one transform for GROW and SHRINK, two for OPEN and CLOSE, whatever the radius.  out (may be NULL) holds the
 * statistics of the new mask as vx_segment_edit reports them (rounds = brick_visits = 0, converged = 1).  It drops the island
 * table and the distance field; the accumulator, the frame state, VxCounters, the light grid, the bound tables, the mesh,
 * VxParams, the segment view and what vx_segment_stats and vx_segment_edit_stats report are not touched; with a view on, the
 * next covered call reads the new mask.  Buffers as vx_segment_distance.  VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID,
 * naming the field and changing nothing, before vx_set_params, for NULL params, no current segment, a spacing component that is
 * not finite or <= 0, a radius that is not finite or <= 0, an op outside the enum, band not 0 or 1, band = 1 with another op or
 * with no predicate on this volume, and a volume with more than 16384 voxels along y or z.  group: member 0. */
int vx_segment_margin(VxContext* ctx, const VxMarginParams* params, VxSegmentResult* out);
/* the last vx_segment_distance or vx_segment_margin: kernels launched by the call itself (the mask's statistics apart), and
 * kernel_ms[0 .. 3] = the HIP-event times of the x pass, the y pass, the z pass and the compare-and-pack / the reduction, each
 * summed over the two transforms of OPEN and CLOSE; all 0 before the first call.  Any pointer may be NULL.  group: member 0. */
int vx_distance_stats(VxContext* ctx, uint32_t* launches, double* kernel_ms);

/* ---- the segment store (DESIGN.md section 2 "Segment store"): VX_SEGMENT_SLOTS masks kept on the device beside the current
 * segment, and the calls that need two masks present at once -- the set operations, the comparison of two segmentations and
 * the label map of several.  A slot holds a mask only: one bit per voxel of index_extent (padding included), an allocation
 * of its own of X * Y * Z / 8 bytes made when the slot is first stored to, freed by vx_segment_drop and with the volume (an
 * upload empties the store).  A = the current segment, B = the mask of a slot.  All calls run on the context's stream behind
 * every queued render and synchronise; none touches the accumulator, the frame state, VxCounters, the light grid, the bound
 * tables, the mesh, VxParams, the segment view, the predicate words of the last vx_segment / vx_segment_threshold or what
 * vx_segment_stats reports.  Every call: VX_ERR_INVALID for a NULL ctx, VX_ERR_NO_VOLUME before an upload, VX_ERR_INVALID
 * before vx_set_params, and a refused call changes nothing.  group: member 0. */
#define VX_SEGMENT_SLOTS 32u
/* Copies the current segment into `slot`, replacing what it held; the current segment stays.  VX_ERR_INVALID for
 * slot >= VX_SEGMENT_SLOTS and with no current segment. */
int vx_segment_store(VxContext* ctx, uint32_t slot);
/* Makes the mask of `slot` the current segment (creating one where there was none); the slot keeps its copy.  out (may be
 * NULL) holds the statistics of the mask as vx_segment_write_mask reports them, and vx_segment_edit_stats reports the call
 * (launches = 1).  Drops the island table and the distance field, nothing else.  VX_ERR_INVALID for slot >=
 * VX_SEGMENT_SLOTS and for an empty slot. */
int vx_segment_load(VxContext* ctx, uint32_t slot, VxSegmentResult* out);
/* Frees `slot`; VX_OK for a slot that is empty already.  VX_ERR_INVALID for slot >= VX_SEGMENT_SLOTS. */
int vx_segment_drop(VxContext* ctx, uint32_t slot);
/* occupied: bit k is set when slot k holds a mask.  VX_ERR_INVALID for NULL occupied. */
int vx_segment_slots(VxContext* ctx, uint32_t* occupied);
typedef enum VxCombineOp {
  VX_COMBINE_UNION = 0,       /* A | B                                            */
  VX_COMBINE_INTERSECT = 1,   /* A & B                                            */
  VX_COMBINE_SUBTRACT = 2,    /* A & ~B                                           */
  VX_COMBINE_XOR = 3,         /* A ^ B                                            */
  VX_COMBINE_INVERT = 4       /* ~A over index_extent; slot is ignored            */
} VxCombineOp;
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxCombineParams {
  int32_t op;              /* VxCombineOp                                                                          */
  uint32_t slot;           /* B; ignored by INVERT                                                                 */
} VxCombineParams;
/* Rewrites the current segment in place as op(A, B) with one word-wise kernel.  out (may be NULL) holds the statistics of the
 * new mask as vx_segment_write_mask reports them (rounds = brick_visits = 0, converged = 1); vx_segment_edit_stats reports
 * the call (launches = 1).  Drops the island table and the distance field, nothing else; the slot is not changed; with a view
 * on, the next covered call reads the new mask.  VX_ERR_INVALID for NULL params, an op outside the enum, no current segment
 * (INVERT included), and -- for every op but INVERT -- slot >= VX_SEGMENT_SLOTS or an empty slot. */
int vx_segment_combine(VxContext* ctx, const VxCombineParams* params, VxSegmentResult* out);
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxCompareParams {
  uint32_t slot;           /* B                                                                                    */
  int32_t hausdorff;       /* 0: the overlap counts only; 1: the two directed Hausdorff distances as well          */
  float spacing[3];        /* as VxDistanceParams; read with hausdorff = 1 only                                    */
} VxCompareParams;
/* count_a, count_b, count_and: |A|, |B|, |A & B|, exact (Dice = 2 and / (a + b), Jaccard = and / (a + b - and): the hosts
 * derive them).  With hausdorff = 1, d2_ab = the largest D2_B(i) over i in A and d2_ba = the largest D2_A(i) over i in B, D2_S
 * the uncapped squared distance transform of S with the bits vx_segment_distance gives, and argmax_ab / argmax_ba (x, y, z)
 * the first voxel in C order over (z, y, x) that attains it.  A direction whose own set is empty reports 0 and (0, 0, 0); one
 * whose own set is not empty while the other set is reports +inf and the first voxel of its own set.  The Hausdorff distance is
 * sqrt(max(d2_ab, d2_ba)); the device takes no square root.  With hausdorff = 0 the five are 0.
 * every member is 4 or 8 bytes wide, no padding */
typedef struct VxCompareResult {
  uint64_t count_a, count_b, count_and;
  float d2_ab, d2_ba;
  uint32_t argmax_ab[3], argmax_ba[3];
} VxCompareResult;
/* Compares the current segment with the mask of a slot; neither, nor the island table, is changed.  hausdorff = 0 counts the
 * overlap (a popcount kernel and its reduction), has no limit on the extent and leaves the distance field alone.
 * hausdorff = 1 adds two uncapped transforms (of B, then of A) in the buffers of vx_segment_distance, each followed by a
 * reduction over the voxels of the other set: it overwrites the field, so vx_distance_read is refused afterwards, and
 * vx_distance_stats reports the call's two transforms summed per pass (launches = 10).  out may be NULL.  VX_ERR_INVALID for
 * NULL params, slot >= VX_SEGMENT_SLOTS, an empty slot, no current segment, hausdorff not 0 or 1 and, with hausdorff = 1, a
 * spacing component that is not finite or <= 0 and a volume with more than 16384 voxels along y or z. */
int vx_segment_compare(VxContext* ctx, const VxCompareParams* params, VxCompareResult* out);
/* The label map of n = 1 .. VX_SEGMENT_SLOTS slots, dense (Z, Y, X) uint8 in C order: labels[i] = k + 1 for the first k with
 * voxel i in slots[k], 0 when no listed slot holds it; nvoxels must be X * Y * Z of index_extent.  overlaps (may be NULL): the
 * number of voxels that more than one listed slot holds.  The current segment is not read (none is needed) or changed.  The
 * device buffer, 1 B per voxel, is allocated by the first call and freed with the volume.  VX_ERR_INVALID for NULL slots or
 * labels, n outside 1 .. VX_SEGMENT_SLOTS, a listed slot >= VX_SEGMENT_SLOTS, an empty one, a slot listed twice (duplicate)
 * and a wrong nvoxels. */
int vx_segments_labelmap(VxContext* ctx, const uint32_t* slots, uint32_t n, uint8_t* labels, uint64_t nvoxels, uint64_t* overlaps);

/* ---- histograms (DESIGN.md section 2 "Histograms"): the density histogram, the moments and the exact order statistics of a
 * region, on the device.  Read-only: the call changes nothing but its own buffers.
 *
 * Region.  R = the voxels i of index_extent (padding included, as everywhere in the segment chain) inside the inclusive voxel
 * box [box_lo, box_hi] (VxSegmentParams' meaning, VX_SEGMENT_BOX_END included; the renderer's clip box does not apply) that
 * `source` selects: VX_HIST_VOLUME every voxel of the box (no segment is needed), VX_HIST_SEGMENT the voxels of the current
 * segment, VX_HIST_SLOT those of slot `slot` of the segment store.  d(i) is the density vx_segment thresholds:
 * (volume_density_scale * v(i)) * volume_inv_maj of the last vx_set_params, the same bits on every layout.
 *
 * Two bin rules, one kernel.
 * VX_HIST_LINEAR, lo < hi finite and bins = B in 1 .. VX_HIST_MAX_BINS: the library computes inv = fl32(fl32(B) / fl32(hi - lo))
 * once on the host.  A voxel with d < lo counts in `below`, one with d > hi in `above`; otherwise
 *   bin = min(B - 1, (uint32_t)fl32(fl32(d - lo) * inv)),
 * two fp32 operations rounded to nearest, never contracted.  d == hi lands in the last bin (np.histogram's convention).  Both
 * operations are monotone in d (a rounded subtraction of a constant and a rounded product with a positive constant never
 * reverse an order), so the bins are monotone in d and cumulative counts mean what they say.  A range so narrow that inv is
 * not finite is refused.
 * VX_HIST_KEY, prefix_bits = p in 0 .. 31, key_bits = b in 1 .. VX_HIST_MAX_KEY_BITS, p + b <= 32, prefix < 2^p (0 when p = 0):
 * key(d) = the bits of d as an unsigned integer with the order of the floats (negative: all bits flipped; otherwise: the sign
 * bit set; -0 below +0).  With top = p ? key >> (32 - p) : 0, a voxel with top < prefix counts in `below`, one with top > prefix
 * in `above`, otherwise bin = (key >> (32 - p - b)) & (2^b - 1); there are 2^b bins.  Three calls (11, 11 and 10 bits, each
 * with the prefix the last one found) are a radix select: the hosts derive the exact k-th smallest density of R from them.
 *
 * Result.  counts[ncounts] receives the bins; ncounts must equal the number of bins.  Always
 * below + above + sum(counts) == count == |R|.  With moments = 1, d_sum and d_sum2 are the float64 sums of (double)d and
 * (double)d * (double)d over ALL of R (not only the voxels in range), added in a fixed order -- per brick in the order of
 * vx_segment's sum, then a fixed tree over the per-brick partials -- and d_min / d_max run over R: two calls return the same
 * bytes, and d_sum of a segment equals VxSegmentResult::d_sum bit for bit.  With moments = 0 the four fields are 0 and their
 * kernels do not run (the radix passes).  An empty R is legal: everything is 0. */
typedef enum VxHistSource {
  VX_HIST_VOLUME = 0,    /* every voxel of the box                             */
  VX_HIST_SEGMENT = 1,   /* the current segment                                */
  VX_HIST_SLOT = 2       /* slot `slot` of the segment store                   */
} VxHistSource;
typedef enum VxHistRule {
  VX_HIST_LINEAR = 0,    /* bins of equal width over [lo, hi]                  */
  VX_HIST_KEY = 1        /* key_bits bits of the order key under a prefix      */
} VxHistRule;
#define VX_HIST_MAX_BINS 4096u
#define VX_HIST_MAX_KEY_BITS 12u
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxHistogramParams {
  int32_t source;          /* VxHistSource                                                                         */
  uint32_t slot;           /* VX_HIST_SLOT only                                                                    */
  uint32_t box_lo[3];      /* inclusive voxel box, as VxSegmentParams                                              */
  uint32_t box_hi[3];      /* or VX_SEGMENT_BOX_END per axis: to the far face                                      */
  int32_t rule;            /* VxHistRule                                                                           */
  uint32_t bins;           /* LINEAR: B, 1 .. VX_HIST_MAX_BINS                                                     */
  float lo, hi;            /* LINEAR: the range, lo < hi, finite                                                   */
  uint32_t prefix;         /* KEY: the top prefix_bits bits a counted key must have                                */
  uint32_t prefix_bits;    /* KEY: p, 0 .. 31                                                                      */
  uint32_t key_bits;       /* KEY: b, 1 .. VX_HIST_MAX_KEY_BITS; 2^b bins                                          */
  int32_t moments;         /* 1: d_sum, d_sum2, d_min, d_max as well; 0: they read 0                               */
} VxHistogramParams;
/* every member is 4 or 8 bytes wide, no padding */
typedef struct VxHistogramResult {
  uint64_t count, below, above;
  double d_sum, d_sum2;
  float d_min, d_max;
} VxHistogramResult;
/* The histogram of R.  Runs on the context's stream behind every queued render and synchronises.  It changes nothing: not
 * the segment, its predicate, the slots, the island table, the distance field, the mesh, the segment view, the accumulator,
 * the frame state, VxCounters, VxParams, or what any other *_stats call reports.  Its buffers -- the 64-bit bin array and
 * 24 B of partial moments per brick -- are allocated by the first call and freed with the volume.  out may be NULL.
 * VX_ERR_INVALID for a NULL ctx; VX_ERR_NO_VOLUME before an upload; VX_ERR_INVALID, naming the field and changing nothing,
 * before vx_set_params, for NULL params, a source or rule outside its enum, SEGMENT with no current segment, SLOT with
 * slot >= VX_SEGMENT_SLOTS or an empty slot, a box that is empty or outside the volume, LINEAR with bins outside
 * 1 .. VX_HIST_MAX_BINS, lo or hi not finite, lo >= hi or a range too narrow for a finite inv, KEY with key_bits outside
 * 1 .. VX_HIST_MAX_KEY_BITS, prefix_bits > 31, prefix_bits + key_bits > 32 or prefix >= 2^prefix_bits, ncounts that is not
 * the number of bins, NULL counts, and moments that is not 0 or 1.  group: member 0. */
int vx_histogram(VxContext* ctx, const VxHistogramParams* params, uint64_t* counts, uint32_t ncounts, VxHistogramResult* out);
/* The last vx_histogram: launches = the kernels it launched (1, or 2 with moments), kernel_ms[0 .. 1] = the HIP-event times
 * of the histogram pass and of the moments' reduction; all 0 before the first call.  Any pointer may be NULL.  group:
 * member 0. */
int vx_histogram_stats(VxContext* ctx, uint32_t* launches, double* kernel_ms);

/* ---- segment views (DESIGN.md section 2 "Segment views"): show only, or hide, the current segment.  With a view other than
 * OFF the covered calls -- vx_render_frame / vx_render_frames in VX_MODE_DVR, _DVR_PHONG, _MIP and _MINIP, and vx_isosurface
 * (hence picking) -- sample the masked volume: every decoded voxel v(i) reads +0.0f where it is hidden (ONLY: i is not in the
 * segment; HIDE: i is in it) and exactly what it reads today elsewhere.  The image is, bit for bit, that of a volume whose hidden
 * voxels decode to 0.  Masked launches run without range skipping (dvr_skip_empty and VxIsoParams::skip are ignored; the
 * isosurface reports skipped = 0).  vx_slice, vx_slice_segment_mask and vx_segment keep reading the unmasked data.  With the view
 * on, a covered call returns VX_ERR_INVALID, naming the reason, for a path-traced render mode, debug_hits, dvr_shadow_stride != 0,
 * a launch without an LDS-window kernel (a REFERENCE or CELLQUAD layout for DVR and the projections, dvr_ert_tau <= 0, a TF
 * longer than the LDS holds, VX_DVR_KERNEL=generic) and no current segment.  An upload drops the segment and resets the view to
 * OFF; a new vx_segment replaces the mask the next covered call reads. */
typedef enum VxSegmentView {
  VX_SEGVIEW_OFF = 0,   /* default: the unmasked volume                       */
  VX_SEGVIEW_ONLY = 1,  /* the segment alone: voxels outside it read 0         */
  VX_SEGVIEW_HIDE = 2   /* everything but the segment: its voxels read 0       */
} VxSegmentView;
/* VX_ERR_INVALID for a value outside VxSegmentView, a device group (the segment lives on member 0 only), and ONLY / HIDE with no
 * current segment.  Host state only: nothing is launched; the accumulator is the caller's to restart. */
int vx_set_segment_view(VxContext* ctx, int view);
/* the current view (VX_SEGVIEW_OFF after an upload); VX_ERR_INVALID for NULL view */
int vx_get_segment_view(VxContext* ctx, int* view);

/* ---- meshes (no reference counterpart; DESIGN.md section 2 "Meshes"): the surface of an isosurface or of the current segment
 * as an indexed triangle mesh, by naive surface nets -- one vertex per grid cell the surface passes through, one quad (two
 * triangles) per grid edge it crosses.
 *   DENSITY  f(i) = d(i) of vx_segment (the last vx_set_params), inside(i) = f(i) >= iso, the comparison vx_isosurface makes
 *   SEGMENT  inside(i) = the bit of the current segment, f = inside ? 1 : 0, iso = 0.5: every crossing at the middle of its edge
 * Every voxel outside [box_lo, box_hi] (VxSegmentParams' meaning, VX_SEGMENT_BOX_END included) or outside index_extent is outside
 * with f = 0, so a mesh is closed where a structure meets the box or a face of the volume.  The renderer's clip box does not apply.
 * Cell c (c_a in [-1, extent_a - 1]) has the corners c + {0, 1}^3; one with a crossing edge owns the vertex c + (the fp32 mean of
 * its crossings), in voxel-centre coordinates (voxel i at i; a host adds 1/2 for index space).  Vertex and triangle order are a
 * function of the input only: two calls, and every layout, give the same bytes.  Triangles wind so that the normal points from
 * inside to outside: the signed volume of a mesh is positive. */
typedef enum VxMeshSource {
  VX_MESH_DENSITY = 0,
  VX_MESH_SEGMENT = 1
} VxMeshSource;
/* every member is 4 bytes wide, no padding (parsed like VxParams by the hosts) */
typedef struct VxMeshParams {
  int32_t source;          /* VxMeshSource                                                                         */
  float iso;               /* DENSITY: finite, > 0; SEGMENT: ignored                                               */
  uint32_t box_lo[3];      /* inclusive voxel box inside index_extent, box_lo <= box_hi                           */
  uint32_t box_hi[3];      /* or VX_SEGMENT_BOX_END per axis: to the far face                                      */
  uint32_t max_vertices;   /* 0 = 2^32 - 2                                                                         */
  uint32_t max_triangles;  /* 0 = 2^32 - 2                                                                         */
} VxMeshParams;
/* blocks: the cell blocks of the volume (8^3 cells each, one more than bricks per axis); active_blocks: those with an active
 * cell.  bbox: the inclusive cell box of the active cells, all 0 when the mesh is empty; a component is an int32_t in two's
 * complement (cells start at -1: 0xffffffff). */
typedef struct VxMeshResult {
  uint64_t vertices, triangles, active_blocks, blocks;
  uint32_t bbox_lo[3], bbox_hi[3];
} VxMeshResult;
/* Builds the context's one mesh on the device, on the context's stream behind every queued render, and synchronises.  out may
 * be NULL.  An empty mesh is no error.  The accumulator, the frame state, VxCounters, the light grid, the bound tables, VxParams,
 * the current segment and the segment view are not touched.  Reads the layout resident at the call (all layouts give the same
 * bits).  Its buffers (64 B per brick, 64 B + 2 x 8 B per cell block) are allocated on first use, the outputs (24 B per vertex,
 * 12 B per triangle) grow to the largest mesh, and all are freed with the volume; an upload drops the mesh.  VX_ERR_NO_VOLUME
 * before an upload; VX_ERR_INVALID, naming the field, before vx_set_params, for NULL params, an unknown source, iso not finite
 * or <= 0 (DENSITY), a box that is empty or outside the volume, SEGMENT with no current segment, and a mesh of more than
 * max_vertices / max_triangles (the message carries both counts; no mesh is kept, the previous one is dropped too).  Any other
 * refused call changes nothing.  group: member 0. */
int vx_mesh_extract(VxContext* ctx, const VxMeshParams* params, VxMeshResult* out);
/* the current mesh: 3 floats and 3 cell components per vertex, 3 vertex indices per triangle.  Any pointer may be NULL.
 * VX_ERR_INVALID with no current mesh. */
int vx_mesh_read(VxContext* ctx, float* verts_xyz, int32_t* cells_xyz, uint32_t* tris);
/* the last vx_mesh_extract: kernels launched (the same for every mesh) and the HIP-event times of the inside words, of the
 * active cells with their scan, and of the emission, kernel_ms[0 .. 2]; all 0 before the first call.  group: member 0. */
int vx_mesh_stats(VxContext* ctx, uint32_t* launches, double* kernel_ms);

/* test hook (no reference counterpart): the device's R8-unorm decode table, 256 floats */
int vx_debug_unorm_table(VxContext* ctx, float* out256);
/* test hook: the host-built empty-space bitmask (pure CPU; bits_out may be NULL to query level/dims) */
int vx_debug_build_skip_mask(const uint32_t* range_packed, const uint32_t brick_count[3], const float* tf_rgba,
                             uint32_t tf_len, const VxParams* params, uint32_t* bits_out, uint32_t* level_out,
                             uint32_t dims_out[3]);
/* test hook: the host-built density bounds of range skipping (VX_MODE_MIP / VX_MODE_MINIP; pure CPU, no context).  Per
 * macro cell of the empty-space grid (the level and dims vx_debug_build_skip_mask reports for the same brick grid), two
 * floats {lo, hi}: every density d = trilinear(q) * volume_inv_maj that a sample q of the cell can produce on the device lies
 * in [lo, hi].  With volume_density_scale <= 0 or volume_inv_maj <= 0 (or either not finite) the bounds are {-inf, +inf}:
 * nothing is skipped.  bounds_out holds 2 * dims[0] * dims[1] * dims[2] floats, or is NULL to query level / dims. */
int vx_debug_build_projection_bounds(const uint32_t* range_packed, const uint32_t brick_count[3], const VxParams* params,
                                     float* bounds_out, uint32_t* level_out, uint32_t dims_out[3]);
/* test hook: which 16x16-pixel blocks of a width x height image no primary DVR ray can hit the clip box from (pure CPU, no
 * context): flags_out[by * ceil(width / 16) + bx] = 1 for such a block, 0 where a ray may hit; *n_out = how many are 1.  The
 * proof needs a perspective camera in front of all eight corners of volume_aabb_min .. max and finite matrices; without it, or
 * with VX_DVR_MISS=0 in the environment, no block is flagged.  A multi-frame launch of plain DVR on the LDS-window kernel hands the
 * flagged blocks to a light kernel (images and counters do not change).  Either out pointer may be NULL. */
int vx_debug_classify_miss_blocks(const VxParams* params, uint32_t width, uint32_t height, uint8_t* flags_out, uint32_t* n_out);
/* test hook: how many 16x16-pixel blocks per frame the last render launch gave its march kernel and the light kernel of the
 * blocks that cannot hit the clip box (0 when the launch was not split).  group: summed over the members. */
int vx_debug_last_launch_blocks(VxContext* ctx, uint32_t* heavy_out, uint32_t* miss_out);

#ifdef __cplusplus
}
#endif
#endif /* VOLXEL_HIP_H */
