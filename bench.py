#!/usr/bin/env python3
"""bench.py -- headline benchmark: Gsamples/s of the DVR raymarch on BASELINE config 3
(512^3 volume, 1920x1080, trilinear + 1-D TF LUT, early ray termination, clip box).

    python bench.py --gpus N --steps K --warmup W        (N > 1 with no launcher around it: starts its own N ranks, launch_ranks)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N ... bench.py --gpus N ...      (the driver's form)

A "step" is one batch of `--frames-per-step` (32) accumulation frames of the 1080p image -- the unit the host hands
the device (`Volxel3DRenderer.render(frames)` batches 32 frames per launch; the viewer accumulates up to 2000,
viewer.ts:1356) -- every frame one pass of the hot path over every pixel, with the per-frame sub-pixel and start
jitter of the reference (fragment.frag:146, raymarch.glsl:30) ON, so every frame marches its own rays.  (Rounds 1-2
and the first half of round 3 called ONE frame a step: the driver's `--steps 20` then timed a single 4.4 ms launch,
which the round-2 verdict rightly called thin; `--frames-per-step 1` reproduces it.  `value` is samples / time either
way.)  With N > 1 the frame's 64x64 tiles are dealt to the ranks (volume replicated, no
collective in the data path); the exchange step -- an RCCL all_gather of the per-rank slabs -- runs at
display cadence, once per `--gather-every` accumulation frames, on a second HIP stream from a snapshot
of the slab so that it overlaps the next frames.  Strong scaling: the frame is fixed, `value` = samples
of all ranks / max-over-ranks time.

Prints ONE JSON line on rank 0 (contract in the task statement).  Besides the contract keys:
  roofline      the dominant kernel (vx::render_dvr_lds<16>; --layout 1: vx::render_dvr_cq<4>) against the resource the
                counters name as its limit.  The LDS-window kernel is bound by vector-ALU issue (`bound` "valu"): `achieved` =
                the vector instructions the march NEEDS (a hand-derived minimum per sample, NECESSARY_VALU below / DESIGN.md
                section 6, x the samples and transfer-function fetches the kernel counted) / the mean HIP-event duration of
                the timed launches; `peak` = one wave64 instruction per 2 clocks per SIMD x 1024 SIMDs at the nominal clock;
                `frac` = achieved / peak.  `algorithmic_gbs` = the SURVEY 8(d) byte model (16 B per sample + the result
                written) over the same duration -- NOT a roofline fraction: the kernel stages each voxel once per window, so
                the model exceeds what the HBM pins carry (`hbm_measured`, `traffic` = HBM bytes per launch from the rocprofv3
                PMC passes of this same command when profiles/traffic.json holds them for exactly this launch shape, else
                null); `blend` = the merge kernel (fragment.frag:158 applied in order), timed apart; `frames_per_launch_1` =
                the same measurement with one frame per launch;
  roofline.issue  the same limiter from the instructions the kernel actually issued: clocks per wave step per CU (live) against
                VALU instructions per wave step (rocprofv3 SQ_INSTS_VALU of this same command);
  roofline.l1   (--layout 1, the cellquad gather kernel) the vector L1 / texture path: gather instructions counted by
                the kernel, distinct 128-byte lines per gather counted by a probe build of the same kernel,
                clocks per gather per CU, and the floor the L1 sustains for that many line look-ups with no
                arithmetic at all (vx_probe_gather_rate, measured in this run);
  cpu_baseline  the scalar CPU oracle (oracle/, kind "port") timed on this box's host cores.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0      # MI355X_MICROARCH.md: HBM3E peak 8.0 TB/s (spec)
BYTES_PER_SAMPLE = 16.0    # 8 x 1 B voxels + 4 B range + 4 B indirection
BYTES_PER_PIXEL_RESULT = 16.0   # RGBA32F result written by the render kernel (one frame of one launch)
BYTES_PER_PIXEL_BLEND = 32.0    # accumulator read + write by the blend (+32 B per pixel per frame
                                # = this + nothing else when a frame is blended in the render kernel itself)
DEFAULT_FRAMES_PER_LAUNCH = 32
KERNEL = {None: "vx::render_dvr_lds<16>", 0: "vx::render_generic<3,0>", 1: "vx::render_dvr_cq<4>", 2: "vx::render_dvr_lds<16>",
          4: "vx::render_dvr_lds<16,false,false,true>"}
LAYOUT = {None: "brickf32", 0: "reference", 1: "cellquad", 2: "brickf32", 4: "bricku8"}   # None = VX_LAYOUT_AUTO: DVR marches brickf32


def build_scene(width, height, n_vox, rank, world, device):
    from volxel_amd import (BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth)
    t0 = time.time()
    vox, sp = synth.value_noise(n_vox, seed=42)
    t1 = time.time()
    msg = read_u16_stack_to_grid(vox, sp)
    t2 = time.time()
    del vox
    r = Volxel3DRenderer(width, height, device=device, shard_rank=rank, shard_count=world)
    r.setup_from_grid(msg)
    secs, nbytes, pinned = r.upload_stats()
    r.restore_settings(BENCHMARK_SETTINGS)      # TF stops, camera pose, histogram range, multiplier
    r.settings.render_mode = "dvr"
    r.settings.volume_clip_min = (0.25, 0.0, 0.0)
    r.settings.volume_clip_max = (1.0, 1.0, 0.75)
    r.settings.dvr_step_voxels = 0.5
    r.settings.dvr_ert_epsilon = 1e-4
    r.settings.dvr_jitter = True        # distinct rays per accumulation frame, as the reference jitters
    r.settings.dvr_skip_empty = False   # BASELINE config 3 is ERT + clip box; skipping is reported aside
    r.settings.max_samples = 1 << 30
    nb = int(np.prod(msg.indirection_size))
    info = dict(gen_s=round(t1 - t0, 2), brick_build_s=round(t2 - t1, 2),
                upload={"seconds": round(secs, 4), "host_mb": round(nbytes / 1e6, 1),
                        "host_gb_per_s": round(nbytes / secs / 1e9, 2) if secs > 0 else None,
                        "pinned": bool(pinned),
                        "note": "vx_upload_volume: PCIe copies from the caller's pinned pages + device-side "
                                "layout build, overlapped; load-time cost, never inside `value`"},
                bricks=nb, nonconstant_bricks=int(msg.brick_counter))
    return r, msg, info


def cpu_baseline(r, msg, crop=(1920, 1080)):
    """scalar CPU port (the parity oracle) on the same frame (or a centred crop of it),
    on at most 16 host threads (the CPU share of a 1-GPU box)"""
    from oracle import oracle as O
    p = r.bind_uniforms()
    W, H = r.width, r.height
    tf, L = r._tf
    threads = min(os.cpu_count() or 1, 16)
    crop = (min(crop[0], W), min(crop[1], H))
    x0, y0 = (W - crop[0]) // 2, (H - crop[1]) // 2
    vol = O.make_volume(msg)
    env = O.Environment(r.environment.floats, r.environment.width, r.environment.height) if r.environment else None
    t0 = time.perf_counter()
    _, c = O.render(p, vol, tf, L, frame_index=0, rect=(x0, x0 + crop[0], y0, y0 + crop[1]), threads=threads,
                    env=env)
    dt = time.perf_counter() - t0
    # single-thread figure on the centred 480x270 crop (1/16 of 1080p), BASELINE.md section 4
    sw, sh = min(480, W), min(270, H)
    sx, sy = (W - sw) // 2, (H - sh) // 2
    t1 = time.perf_counter()
    _, c1 = O.render(p, vol, tf, L, frame_index=0, rect=(sx, sx + sw, sy, sy + sh), threads=1, env=env)
    dt1 = time.perf_counter() - t1
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            model = next((ln.split(":", 1)[1].strip() for ln in f if ln.startswith("model name")), "")
    except OSError:
        pass
    return {"value": round(c.samples / dt / 1e9, 5), "unit": "Gsamples/s", "cores": threads, "kind": "port",
            "sample": f"centred {crop[0]}x{crop[1]} crop of frame 0 of the same workload (jitter on), {c.samples} samples in "
                      f"{dt:.2f} s ({threads} threads over row bands)",
            "ms_per_frame_crop": round(dt * 1e3, 1),
            "single_thread": {"value": round(c1.samples / dt1 / 1e9, 5), "unit": "Gsamples/s", "cores": 1,
                              "sample": f"centred {sw}x{sh} crop, {c1.samples} samples in {dt1:.2f} s"},
            "cpu_model": model, "host_cores": os.cpu_count()}


def traffic_from_profile(a, frames_per_launch, jitter):
    """HBM bytes per launch from the rocprofv3 PMC passes of this same command (tools/pmc_profile.sh ->
    profiles/traffic.json): 2 x FETCH_SIZE (gfx950 reports half of the fetched bytes, MI355X_MICROARCH.md
    section HBM) + WRITE_SIZE.  Only when the profiled launch shape is exactly the one timed here."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        for t in json.load(open(path)).get(LAYOUT[a.layout], []):
            if (t["width"], t["height"], t["volume"], t["frames_per_launch"], bool(t["dvr_jitter"])) == \
                    (a.width, a.height, a.volume, frames_per_launch, bool(jitter)):
                return {"traffic": int(t["hbm_bytes_per_launch"]), "traffic_source": t["source"], "_entry": t}
    except Exception:
        pass
    return {"traffic": None}


def l1_block(r, c, clock_khz_hint=None):
    """the limiter the counters name: vector L1 / texture path.  Everything is measured in this run:
    gathers (exact, by the kernel), their line spread (probe build of the same kernel on frame 0), the floor
    (nothing-but-gathers kernel at the same number of line look-ups per instruction)."""
    n, lines, quads = r.probe_gather_spread(0)
    if not n or not c.gathers or not c.kernel_ms:
        return None
    name, cus, mem = r.device_info()
    lpg, qpg = lines / n, quads / n
    look = max(16, min(64, int(round(qpg))))
    dist = max(1, min(look, int(round(lpg))))
    floor_clk, khz = r.probe_gather_rate(look, dist)   # the march's look-ups per gather over its distinct lines
    ideal_clk, _ = r.probe_gather_rate(16, min(16, dist))   # every group of 4 lanes inside one line: the best a gather can do
    clk = (c.kernel_ms * 1e-3) * (khz * 1e3) * cus / c.gathers
    return {"bound": "l1", "unit": "clk per gather instruction per CU at the nominal clock",
            "nominal_clock_mhz": round(khz / 1e3, 1),
            "gathers": int(c.gathers // max(c.launches, 1)),
            "bytes_returned_per_gather": 1024,
            "lines_per_gather": round(lpg, 2), "quad_lookups_per_gather": round(qpg, 2),
            "clk_per_gather_per_cu": round(clk, 2), "floor_clk": round(floor_clk, 2),
            # probe and kernel each run at the clock the chip chooses for them: a few per cent either way is DVFS
            # noise, so the fraction saturates at 1 (frac_raw keeps the quotient as measured)
            "frac": round(min(1.0, floor_clk / clk), 4), "frac_raw": round(floor_clk / clk, 4),
            "floor_clk_if_coalesced": round(ideal_clk, 2), "frac_of_coalesced": round(ideal_clk / clk, 4),
            "l1_return_gbs": round(c.gathers * 1024 / (c.kernel_ms * 1e-3) / 1e9, 1),
            "note": "floor_clk = vx_probe_gather_rate(round(quad_lookups_per_gather), round(lines_per_gather)): "
                    "global_load_dwordx4 only, L1-resident, same number of line look-ups per instruction over the same number "
                    "of distinct lines; frac = floor / measured (<= 1, falls "
                    "when the kernel adds stalls); frac_of_coalesced = what a march whose 4-lane groups never "
                    "straddle a line would reach"}


VALU_CLK_PER_INST = 2.0   # MI355X_MICROARCH.md: a wave64 VALU instruction issues over 2 cycles of a SIMD-32
NOMINAL_CLOCK_GHZ = 2.4   # MI355X_MICROARCH.md: max clock 2400 MHz
N_SIMDS = 1024            # 256 CUs x 4 SIMDs
# Vector instructions the bit-exact march cannot do without, per sample and lane (DESIGN.md section 6 derives them):
#   position q = fma(k, dq, q0) per axis 3, floor 3, fraction 3, complement 1 - f 3, tile address 4 (three fmas on the float
#   cells, one conversion), the seven lerps of common.glsl:62-68 as mul + fma 14, density scale and
#   inv_maj 2, sample-range test 2, step count 1                                                          = 35
# and per sample that lies inside the sample range (fetches a transfer-function entry and is composited):
#   LUT index 3 (mul, convert, clamp), address 1, alpha * maj 1, tau fma 1, exp2 argument 1, exp2 1, T_prev - T 1,
#   three colour fmas 3, termination test 1                                                               = 13
NECESSARY_VALU = {"per_sample": 35, "per_tf_sample": 13,
                  "phong_per_shaded_sample": 0}   # (the Phong gradient is not part of the headline workload)
# The same lists priced with the issue rates tools/op_rate.hip measured on the device (profiles/r03_op_rates.txt): 2 clocks
# per wave64 instruction for fp32 fma / mul / add / sub and u32 add, 4 for floor, conversions, compares, selects, clamps
# and shift-adds, 8 for exp2:
#   per sample: fmas of position and address 6 x 2, floor 3 x 4, fraction and complement 6 x 2, conversion 4, lerps 14 x 2,
#   scales 2 x 2, range test 2 x 4, step count 2                                                          = 82 clocks
#   per sample in range: index mul 2 + convert 4 + clamp 4, address 4, alpha * maj 2, tau fma 2, exp2 argument 2, exp2 8,
#   T_prev - T 2, colour fmas 3 x 2, termination compare 4                                                = 40 clocks
NECESSARY_CLK = {"per_sample": 82, "per_tf_sample": 40}


def issue_block(r, c, entry):
    """the limiter of the LDS-window kernel: vector-ALU issue.  Live: wave steps (a wave taking one march step), staging
    loads and LDS tap reads counted by the kernel.  From the rocprofv3 PMC pass of this same command
    (profiles/traffic.json, only for exactly this launch shape): the VALU instructions the kernel issues per launch.
    floor = those instructions at the architectural issue rate (one wave64 instruction per 2 clocks per SIMD, 4 SIMDs
    per CU); the clocks are nominal (the chip runs this kernel at ~2.3 GHz, GRBM_GUI_ACTIVE in the same profile)."""
    if not c.lane_slots or not c.kernel_ms:
        return None
    name, cus, mem = r.device_info()
    fma_clk, khz = r.probe_valu_rate()
    launches = max(c.launches, 1)
    steps = c.lane_slots / 64
    clk = (c.kernel_ms * 1e-3) * (khz * 1e3) * cus / steps
    out = {"bound": "valu", "unit": "clk per wave step (64 lanes x one march step) per CU at the nominal clock",
           "nominal_clock_mhz": round(khz / 1e3, 1),
           "wave_steps": int(steps // launches), "staging_loads_per_wave_step": round(c.gathers / steps, 4),
           "lds_tap_reads_per_wave_step": round(c.lds_reads / steps, 3),
           "clk_per_wave_step_per_cu": round(clk, 2),
           "valu_insts_per_wave_step": None, "clk_per_valu_inst_per_simd": None, "floor_clk": None, "frac": None,
           "pure_fma_stream_clk_per_inst_per_simd": round(fma_clk, 2),
           "note": "floor_clk = VALU instructions per wave step (rocprofv3 SQ_INSTS_VALU of this same command / wave steps) "
                   "x 2 clk / 4 SIMDs; frac = floor / measured; pure_fma_stream = what a stream of independent v_fma_f32 "
                   "reaches on this device in this run (8 waves per SIMD; it is power-limited, so not a ceiling for a mixed stream)"}
    if entry and entry.get("sq_insts_valu_per_launch"):
        per_step = entry["sq_insts_valu_per_launch"] / (steps / launches)
        floor = per_step * VALU_CLK_PER_INST / 4.0
        out.update({"valu_insts_per_wave_step": round(per_step, 1), "clk_per_valu_inst_per_simd": round(clk * 4.0 / per_step, 2),
                    "floor_clk": round(floor, 2), "frac": round(floor / clk, 4),
                    "valu_source": entry["source"].split(" (")[0]})
        if entry.get("effective_clock_mhz"):
            # the clock the chip actually held while running this kernel (GRBM_GUI_ACTIVE / 8 XCDs / traced duration)
            eff = entry["effective_clock_mhz"]
            out.update({"effective_clock_mhz": round(eff, 0),
                        "frac_at_effective_clock": round(floor / (clk * eff * 1e3 / khz), 4)})
    return out


MODE_BYTES_PER_SAMPLE = {"default": 16.0, "no_dda": 16.0, "raymarch": 9.0, "dvr": 16.0, "dvr_phong": 64.0}


def mode_record(mode, c, a):
    """one render mode on the bench scene: kernel time per accumulation frame, its rate, and the SURVEY 8(d) byte roofline
    (bytes per sample by the taps the mode fetches + 4 B per DDA step + 32 B per pixel and frame, over the kernel time and
    the HBM peak).  Lane utilisation comes from the committed PMC profile of this launch shape, when there is one."""
    frames = max(int(c.frames), 1)
    ms = c.kernel_ms / frames
    alg = (c.samples * MODE_BYTES_PER_SAMPLE[mode] + c.skip_steps * 4.0 + c.pixels * BYTES_PER_PIXEL_BLEND) / frames
    gbs = alg / (ms * 1e-3) / 1e9 if ms > 0 else 0.0
    rec = {"ms_per_frame": round(ms, 4),
           "samples_per_frame": int(c.samples // frames),
           "dda_steps_per_frame": int(c.skip_steps // frames),
           "rays_per_frame": int(c.rays // frames),
           "gsamples_per_s": round(c.samples / (c.kernel_ms * 1e-3) / 1e9, 2) if c.kernel_ms else None,
           "frames_per_launch": int(c.max_launch_frames),
           "roofline": {"bound": "hbm", "unit": "GB/s", "model": "algorithmic bytes (SURVEY 8(d))",
                        "bytes_per_sample": MODE_BYTES_PER_SAMPLE[mode], "algorithmic_bytes_per_frame": int(alg),
                        "achieved": round(gbs, 1), "peak": HBM_PEAK_GBS, "frac": round(gbs / HBM_PEAK_GBS, 4),
                        **({"above_peak": "the byte model charges every tap to HBM; this kernel takes its taps from LDS windows "
                                          "staged once (vx_dvr_lds.hpp), so the model exceeds what the HBM pins carry: "
                                          "not a roofline fraction, see the top-level roofline for the limiter"}
                           if gbs > HBM_PEAK_GBS else {})},
           "lane_utilisation": (round((c.active_lane_slots or c.samples) / c.lane_slots, 4) if c.lane_slots else None),
           "lane_utilisation_source": (("counted by the kernel: march-loop trips of the lanes / 64 x the trips of each wave's slowest lane "
                                        "(primary + shadow segment; exact at bounces 1)") if c.active_lane_slots else
                                       "counted by the kernel (samples / lane slots of the march)") if c.lane_slots else None}
    try:
        prof = json.load(open(os.path.join(ROOT, "profiles", "modes.json")))
        e = prof.get(mode)
        if e and (e["width"], e["height"], e["volume"]) == (a.width, a.height, a.volume):
            # the committed PMC profile of this scene beside the live count: active lanes over ALL issued vector instructions
            rec["lane_utilisation_pmc"] = e["lane_utilisation"]
            rec["lane_utilisation_pmc_source"] = e["source"]
            if rec["lane_utilisation"] is None:
                rec["lane_utilisation"], rec["lane_utilisation_source"] = e["lane_utilisation"], e["source"]
            for k in ("hbm_bytes_per_frame", "l1_hit", "l2_hit", "valu_issue_of_clocks"):
                if k in e:
                    rec[k] = e[k]
    except Exception:
        pass
    return rec


def workload_name(a, world):
    """BASELINE.json `configs` index of the workload (configs[2] = config 3 is the one `metric` is quoted on)"""
    shape = (a.volume, a.width, a.height)
    if shape == (512, 1920, 1080):
        return "config3" if world == 1 else f"config3 workload, image tiles over {world} GPUs"
    if shape == (1024, 3840, 2160):
        return "config5" if world == 8 else f"config5 workload on {world} GPU" + ("s" if world > 1 else "")
    return "custom"


def launch_plan(first, count, per_launch, gather_every):
    """`count` accumulation frames first.. as equal launches of at most `per_launch` frames (20 frames at 16 per launch go
    as 10 + 10); a launch is followed by the exchange step when its last frame completes a group of `gather_every`
    frames (display cadence).  Returns [(first frame, frames, exchange afterwards)] -- tests/test_bench_plan.py."""
    plan, done = [], 0
    while done < count:
        launches_left = -(-(count - done) // per_launch)
        n = -(-(count - done) // launches_left)
        f0 = first + done
        plan.append((f0, n, (f0 + n) // gather_every != f0 // gather_every))
        done += n
    return plan


DUMP_FULL_MAX_BYTES = 48 << 20     # --dump-outputs: larger images are sampled (the dump stays under 64 MB)
DUMP_SAMPLE_PIXELS = 1 << 20


def dump_outputs(out_dir, accum, c):
    """--dump-outputs: the accumulated image of the timed run and its counters as float32 / float64 .npy files.  An image
    above DUMP_FULL_MAX_BYTES is reduced to DUMP_SAMPLE_PIXELS pixels drawn by a fixed seed (accum_index.npy holds their
    flat pixel indices), so two builds of the same command dump the same pixels."""
    os.makedirs(out_dir, exist_ok=True)
    accum = np.ascontiguousarray(accum, dtype=np.float32)
    if accum.nbytes > DUMP_FULL_MAX_BYTES:
        h, w, ch = accum.shape
        idx = np.sort(np.random.default_rng(0).choice(h * w, size=DUMP_SAMPLE_PIXELS, replace=False))
        np.save(os.path.join(out_dir, "accum_index.npy"), idx.astype(np.float64))
        accum = accum.reshape(h * w, ch)[idx]
    np.save(os.path.join(out_dir, "accum.npy"), accum)
    np.save(os.path.join(out_dir, "counters.npy"),
            np.array([c.samples, c.tf_samples, c.frames, c.pixels], dtype=np.float64))


def launch_ranks(n, argv):
    """`python bench.py --gpus N` without a launcher around it: start the N ranks the way the driver does
    (`python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py ...`)
    as a CHILD process and return its exit code.  Rank 0's JSON line reaches stdout through the inherited descriptor.
    If the ranks cannot start or any of them fails the code is non-zero: there is no fall-back to fewer ranks."""
    import socket
    import subprocess
    with socket.socket() as s:                 # a free rendezvous port on the loopback interface
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}",
           "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__), *argv]
    sys.stderr.write(f"bench.py: launching {n} ranks: {' '.join(cmd)}\n")
    sys.stderr.flush()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")     # dmabuf IPC: the only mode the host driver supports (RCCL)
    try:
        return subprocess.run(cmd, env=env).returncode or 0
    except OSError as e:
        sys.stderr.write(f"bench.py: could not start the ranks: {e}\n")
        return 1


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20, help="timed steps; a step = --frames-per-step accumulation frames")
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--frames-per-step", type=int, default=32,
                    help="accumulation frames per step (one batch of the host: Volxel3DRenderer.render(frames) hands the device "
                         "32 frames per launch); 1 = the step of rounds 1-2")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1080)
    ap.add_argument("--volume", type=int, default=512)
    ap.add_argument("--no-cpu-baseline", action="store_true")
    ap.add_argument("--layout", type=int, default=None,
                    help="0 reference, 1 cellquad (gather kernel), 2 brickf32 (LDS-window kernel), 4 bricku8 (the same kernel, 8-bit bricks "
                         "decoded while a window is staged); default: the library's "
                         "VX_LAYOUT_AUTO, which marches DVR on brickf32")
    ap.add_argument("--gather-every", type=int, default=64,
                    help="N>1: all_gather the framebuffer once per this many accumulation frames")
    ap.add_argument("--frames-per-launch", type=int, default=None,
                    help="independent accumulation frames rendered by one kernel launch (1..64); default 32 x the "
                         "number of ranks, at most 64 (what the library takes per launch)")
    ap.add_argument("--precondition-ms", type=float, default=0.0,
                    help="diagnostic, off by default: keep the device busy with untimed frames of the same workload for this long "
                         "before the W warm-up steps (an MI355X drops its clocks within a millisecond of idling: tools/fpl_sweep.py "
                         "--sync).  With 32-frame steps the 5 warm-up steps are 35 ms of load and the timed region 135 ms: measured "
                         "1005 Gsamples/s without and 1007 with 150 ms of preconditioning; with --frames-per-step 1 (a 4.4 ms timed "
                         "region) it was 800 against 965.  When on it is reported as config.preconditioning and value_cold = the "
                         "same W + K steps measured before it")
    ap.add_argument("--no-cold", action="store_true", help="skip the un-preconditioned pass that yields value_cold")
    ap.add_argument("--no-jitter", action="store_true",
                    help="diagnostic: pixel-centre rays, identical in every frame (NOT the reference's behaviour)")
    ap.add_argument("--no-skip-variant", action="store_true", help="do not run the secondary measurement with skipping")
    ap.add_argument("--no-mode-variants", action="store_true", help="do not time the other render modes afterwards")
    ap.add_argument("--no-side-measurements", action="store_true",
                    help="skip the 1-frame-per-launch run and the L1 probes (profiling passes)")
    ap.add_argument("--force-gather", action="store_true", help="run the gather path with one rank too (testing)")
    ap.add_argument("--rehearse-gloo", action="store_true",
                    help="TEST MODE, not a measurement: run the N ranks of --gpus N on ONE device with the gloo backend (RCCL "
                         "refuses several ranks on one GPU): everything of the N > 1 path -- tile dealing, balanced order, sharded "
                         "contexts, launch plan, snapshot + all_gather + de-tile, the reductions of the line -- except RCCL itself; "
                         "the collectives are staged through host memory.  The line says \"rehearsal\" and carries the sha256 of the "
                         "gathered image (config.image_sha256: equal to a 1-rank --force-gather run of the same frames)")
    ap.add_argument("--no-balance", action="store_true",
                    help="N>1: keep the default round-robin dealing of the 64x64 tiles instead of the cost-balanced order")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what they computed as DIR/<name>.npy (rank 0): accum.npy = the "
                         "accumulated RGBA32F image (a fixed seeded sample of its pixels when the image exceeds 48 MB, "
                         "with accum_index.npy), counters.npy = rank 0's samples, tf_samples, frames, pixels of the timed run")
    a = ap.parse_args()

    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        # `python bench.py --gpus N` on its own: this process becomes the launcher of N ranks and never touches the GPU
        # (no torch import, no HIP call before or after the spawn; a child process, never an exec)
        raise SystemExit(launch_ranks(a.gpus, sys.argv[1:]))

    # the contract is ONE JSON line on stdout: keep a private handle to the real stdout and send
    # everything else written to fd 1 (RCCL prints a version banner there) to stderr
    sys.stdout.flush()
    real_stdout = os.fdopen(os.dup(1), "w")
    os.dup2(2, 1)

    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    if world != a.gpus:
        # never report a run of `world` ranks as one of `--gpus` GPUs
        raise SystemExit(f"--gpus {a.gpus} but WORLD_SIZE={world}")
    if not torch.cuda.is_available():
        raise SystemExit(f"bench.py needs an MI355X: the HIP path has no CPU fallback (rank {rank} of {world})")
    rehearse = bool(a.rehearse_gloo)
    if torch.cuda.device_count() < (local + 1) and not rehearse:
        raise SystemExit(f"rank {rank} of {world}: no GPU {local} on this node ({torch.cuda.device_count()} visible)")
    if rehearse:
        local = local % max(torch.cuda.device_count(), 1)      # the ranks share the device(s) there are
    torch.cuda.set_device(local)
    use_dist = world > 1 or a.force_gather
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        if rehearse:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local))

    def barrier():
        if rehearse:
            dist.barrier()
        else:
            dist.barrier(device_ids=[local])

    def all_reduce_(t, op):
        """all_reduce of a small CUDA tensor (gloo rehearsal: through host memory)"""
        if rehearse:
            h = t.cpu()
            dist.all_reduce(h, op=op)
            t.copy_(h)
        else:
            dist.all_reduce(t, op=op)
        return t

    r, msg, info = build_scene(a.width, a.height, a.volume, rank, world, local)
    if a.no_jitter:
        r.settings.dvr_jitter = False
    if a.layout is not None:
        r.set_layout(a.layout)
    r.bind_uniforms()
    if world > 1 and not a.no_balance:
        # every rank probes the same tile costs on its own GPU and derives the same dealing order:
        # no communication, equal tile counts per rank, the gathered image stays bit-identical
        r.balance_tiles()
        r.bind_uniforms()

    gathered = image = slab = snap = None
    rs = cs = None
    state = {"copy_done": None, "work": None, "gathers": 0}
    if use_dist:
        from volxel_amd.dist import slab_tensor
        rs, cs = torch.cuda.Stream(), torch.cuda.Stream()    # render / communication streams
        r.set_stream(rs.cuda_stream)
        slab = slab_tensor(r)
        snap = torch.empty_like(slab)
        gathered = torch.empty(world * slab.numel(), dtype=torch.float32, device="cuda")
        image = torch.empty(a.height * a.width * 4, dtype=torch.float32, device="cuda")

    P = max(1, min(64, a.frames_per_launch if a.frames_per_launch else DEFAULT_FRAMES_PER_LAUNCH * world))
    F = max(1, a.frames_per_step)
    frames_timed, frames_warm = a.steps * F, max(a.warmup * F, 2)

    def batch(f0, n, per_launch, exchange):
        """n accumulation frames f0.. (n <= per_launch): one launch, then -- at display cadence -- the gather"""
        if state["copy_done"] is not None:        # the snapshot copy must have read the slab
            rs.wait_event(state["copy_done"])
            state["copy_done"] = None
        r.render(frames=n, rebind=False, in_flight=per_launch)
        if use_dist and exchange:
            gather()

    def gather():
        """snapshot of this rank's slab -> all_gather on the communication stream (overlaps the next launch)"""
        ev = torch.cuda.Event()
        ev.record(rs)
        cs.wait_event(ev)
        with torch.cuda.stream(cs):
            if state["work"] is not None:
                state["work"].wait()          # previous gather no longer reads snap / gathered
            snap.copy_(slab, non_blocking=True)
            done = torch.cuda.Event()
            done.record(cs)
            state["copy_done"] = done
            if rehearse:                      # gloo has no CUDA all_gather: through host memory, synchronously
                host = snap.cpu()
                out = torch.empty(world * host.numel(), dtype=host.dtype)
                dist.all_gather_into_tensor(out, host)
                gathered.copy_(out)
            else:
                state["work"] = dist.all_gather_into_tensor(gathered, snap, async_op=True)
            state["gathers"] += 1

    def fence():
        """barrier + device synchronisation (the contract's bracket): ONE device-wide synchronisation -- it covers the
        library's render stream, the communication stream and the pending all_gather -- then the barrier"""
        tt = [time.perf_counter()]
        if state["work"] is not None:
            state["work"].wait()              # orders the current stream behind the collective (no host wait)
        torch.cuda.synchronize(); tt.append(time.perf_counter())
        if use_dist:
            barrier()                         # returns when every rank has arrived (it synchronises its own stream)
        tt.append(time.perf_counter())
        if os.environ.get("VX_BENCH_TRACE"):
            sys.stderr.write("fence: " + " ".join(f"{(b - a) * 1e3:.3f}" for a, b in zip(tt, tt[1:])) + " ms\n")

    def run(first, count, need_image=False, per_launch=P):
        plan = launch_plan(first, count, per_launch, a.gather_every)
        for f0, n, exchange in plan:
            batch(f0, n, per_launch, exchange)
        if need_image and use_dist and plan and not plan[-1][2]:
            gather()                          # a timed run delivers the image of ALL its frames

    if use_dist:
        # RCCL's first barrier sets the collective up (12 ms measured): here, not in the fence before the timed region,
        # where it would leave the device idle
        barrier()

    def timed(first):
        """W untimed warm-up steps, then EXACTLY a.steps steps (x F accumulation frames) between two fences"""
        # the first two frames (re)build the launch order; the warm-up also performs one gather, so that RCCL's
        # first-use setup of the collective is not inside the timed region
        run(first, frames_warm, need_image=True)
        fence()
        r.reset_counters()
        t0 = time.perf_counter()
        run(first + frames_warm, frames_timed, need_image=True)
        fence()
        dt = time.perf_counter() - t0
        if use_dist:
            t = torch.tensor([dt], dtype=torch.float64, device="cuda")
            all_reduce_(t, dist.ReduceOp.MAX)
            dt = float(t.item())
        return dt, r.counters()

    # (1) COLD: the device as the host left it after generating and uploading the volume (clocks down): `value_cold`
    cold = None
    if a.precondition_ms > 0 and not a.no_cold:
        cold_elapsed, cold_c = timed(0)
        cold = {"elapsed": cold_elapsed, "samples": cold_c.samples}
        r.restart_rendering()
        r.bind_uniforms()
    # device preconditioning: the chip idled while the host generated the volume; a few ms of warm-up steps do not
    # bring it back to the clock it sustains under load (measured: 0.36 instead of 0.31 ms per frame)
    pre = {"frames": 0, "seconds": 0.0}
    if a.precondition_ms > 0:
        t_pre = time.perf_counter()
        while time.perf_counter() - t_pre < a.precondition_ms * 1e-3:
            r.render(frames=P, rebind=False, in_flight=P)
            r.finish()
            pre["frames"] += P
        pre["seconds"] = round(time.perf_counter() - t_pre, 3)
        r.restart_rendering()
        r.bind_uniforms()

    elapsed, c = timed(0)
    n_gathers = state["gathers"]

    # the fixed cost of a timed region that renders nothing: snapshot copy + all_gather + the fences (measured straight
    # after the timed run: device and RCCL in the state the timed region had them)
    fixed_ms = None
    if use_dist:
        fence()
        tf0 = time.perf_counter()
        gather()
        fence()
        fixed_ms = (time.perf_counter() - tf0) * 1e3
        if use_dist:
            t = torch.tensor([fixed_ms], dtype=torch.float64, device="cuda")
            all_reduce_(t, dist.ReduceOp.MAX)
            fixed_ms = float(t.item())

    samples, pixels = c.samples, c.pixels
    cold_samples = cold["samples"] if cold else 0
    if use_dist:
        s = torch.tensor([samples, pixels, cold_samples], dtype=torch.float64, device="cuda")
        all_reduce_(s, dist.ReduceOp.SUM)
        samples, pixels, cold_samples = int(s[0].item()), int(s[1].item()), int(s[2].item())
    image_sha = None
    if use_dist and state["gathers"]:
        # de-tile the last gathered framebuffer so that the image is materialised
        r.detile(gathered.data_ptr(), image.data_ptr())
        r.finish()
        if rank == 0 and (rehearse or a.force_gather):
            import hashlib
            image_sha = hashlib.sha256(image.cpu().numpy().tobytes()).hexdigest()

    if rank == 0 and a.dump_outputs:
        # before the side measurements below render more frames into the accumulator
        # N > 1 (or --force-gather): the de-tiled image of the last gather, which the timed run ends with (need_image)
        accum = image.cpu().numpy().reshape(a.height, a.width, 4) if use_dist else r.read_accum()
        dump_outputs(a.dump_outputs, accum, c)

    if rank == 0:
        name, cus, mem = r.device_info()
        launches = max(c.launches, 1)
        multi = c.max_launch_frames > 1      # multi-frame launches write results; the blend kernel is apart ...
        fused = multi and c.merge_ms == 0.0  # ... unless the render kernel applied the running mean itself (MultiOut::fuse, round 4):
                                             # then a launch reads and writes the accumulator ONCE per pixel, whatever its frames
        px_bytes = (BYTES_PER_PIXEL_BLEND / max(int(c.max_launch_frames), 1)) if fused else \
                   (BYTES_PER_PIXEL_RESULT if multi else BYTES_PER_PIXEL_BLEND)
        alg_bytes_launch = (c.samples * BYTES_PER_SAMPLE + c.pixels * px_bytes) / launches
        avg_kernel_s = c.kernel_ms / launches / 1e3
        achieved = alg_bytes_launch / avg_kernel_s / 1e9 if avg_kernel_s > 0 else 0.0
        fpl = int(c.max_launch_frames)
        prof = traffic_from_profile(a, fpl, r.settings.dvr_jitter)
        prof_entry = prof.pop("_entry", None)
        # the limiter: vector-ALU issue for the LDS-window kernel (rocprofv3: VALU issue ~0.78 of the kernel's clocks, HBM
        # ~0.1 of peak); for the cellquad gather kernel the L1 tag pipe, detailed in roofline.l1 (its top-level figures
        # use the same necessary-instruction count, which does not bind that kernel)
        need = (c.samples * NECESSARY_VALU["per_sample"] + c.tf_samples * NECESSARY_VALU["per_tf_sample"]) / 64.0 / launches
        valu_peak = N_SIMDS * NOMINAL_CLOCK_GHZ / VALU_CLK_PER_INST            # G wave64 instructions per second
        valu_achieved = need / avg_kernel_s / 1e9 if avg_kernel_s > 0 else 0.0
        valu_bound = a.layout in (None, 2, 4)
        issued = prof_entry.get("sq_insts_valu_per_launch") if prof_entry else None
        roof = {
            "bound": "valu" if valu_bound else ("l1" if a.layout == 1 else "latency"),
            # the VALU model only describes the kernel it was derived for: null for the gather / reference-layout kernels
            # (--layout 1: see roofline.l1; --layout 0 has no single limiter)
            "achieved": round(valu_achieved, 1) if valu_bound else None,
            "peak": round(valu_peak, 1) if valu_bound else None, "unit": "G wave64 VALU instructions/s",
            "frac": round(valu_achieved / valu_peak, 4) if valu_bound else None,
            "frac_kind": "model x measurement: NECESSARY vector instructions per sample (a hand-derived count, checked against "
                         "the kernel's ISA listing by tests/test_isa_lint.py) x the samples this run counted / the kernel time "
                         "this run measured; `frac_issued` is the same ratio for the instructions the kernel actually ISSUED "
                         "(rocprofv3 SQ_INSTS_VALU of this command, profiles/traffic.json), idle lanes and overhead included",
            "frac_issued": (round(issued / avg_kernel_s / 1e9 / valu_peak, 4)
                            if (valu_bound and issued and avg_kernel_s > 0) else None),
            "necessary_over_issued": round(need / issued, 4) if (valu_bound and issued) else None,
            "frac_note": "necessary vector instructions (hand-derived minimum of the bit-exact march: 35 per sample and lane + 13 "
                         "per sample inside the sample range, / 64 lanes; per-ray set-up, window placement and idle lanes are "
                         "NOT counted as necessary) per launch / kernel time, against 1024 SIMDs x 2.4 GHz / 2 clocks per instruction",
            "necessary_valu_per_launch": int(need), "necessary_model": NECESSARY_VALU,
            "priced": None if not valu_bound else {
                "frac": round((c.samples * NECESSARY_CLK["per_sample"] + c.tf_samples * NECESSARY_CLK["per_tf_sample"]) / 64.0 / launches
                              / (avg_kernel_s * N_SIMDS * NOMINAL_CLOCK_GHZ * 1e9), 4) if avg_kernel_s > 0 else None,
                "necessary_clk_model": NECESSARY_CLK,
                "note": "the same necessary instructions priced with the issue rates measured on this device (tools/op_rate.hip, "
                        "profiles/r03_op_rates.txt: 2 clocks for fp32 fma / mul / add / sub and u32 add, 4 for floor, conversions, "
                        "compares, selects and clamps, 8 for exp2) over the SIMD clocks of the launch at 2.4 GHz: the share of the "
                        "vector ALUs' time the necessary work would take -- no instruction mix of this march can reach the "
                        "2-clock peak `frac` is quoted against"},
            "tf_samples_per_frame": int(c.tf_samples // max(c.frames, 1)),
            "algorithmic_gbs": round(achieved, 1),
            "algorithmic_gbs_note": "SURVEY 8(d) byte model / kernel time; exceeds the 8000 GB/s HBM peak because the kernel stages "
                                    "each voxel once per window and neighbouring samples share taps -- kept for comparison with "
                                    "earlier rounds, not a roofline fraction",
            **prof,
            "kernel": KERNEL[a.layout],
            "avg_kernel_ms": round(c.kernel_ms / launches, 4), "launches": int(c.launches), "frames": int(c.frames),
            "frames_per_launch": fpl, "min_frames_per_launch": int(c.min_launch_frames),
            "algorithmic_bytes_per_launch": int(alg_bytes_launch),
            "algorithmic_model": f"{int(BYTES_PER_SAMPLE)} B/sample + "
                                 + ("32 B/pixel/launch (the running mean of the launch's frames is applied in the render kernel: "
                                    "one accumulator read + write per pixel and launch)" if fused else
                                    (f"{int(px_bytes)} B/pixel/frame (the result this kernel writes; the blend's 32 B/pixel/frame are in `blend`)"
                                     if multi else f"{int(px_bytes)} B/pixel/frame (accumulator read + write in the same kernel)")),
            "rank0_gsamples_per_s_kernel_only": round(c.samples / (c.kernel_ms / 1e3) / 1e9, 3) if c.kernel_ms else None,
            "hbm_measured": ({"gbs": round(prof["traffic"] / avg_kernel_s / 1e9, 1),
                              "frac": round(prof["traffic"] / avg_kernel_s / 1e9 / HBM_PEAK_GBS, 4),
                              "note": "rocprofv3 bytes of the profiled run of this command / this run's kernel time"}
                             if prof.get("traffic") and avg_kernel_s > 0 else None),
            "blend": {"fused": True, "note": "no blend kernel ran: the render kernel folds the launch's frames into the accumulator in "
                                              "frame order itself (a wave holds every frame of its pixels in launches of exactly 32 / "
                                              "64 frames; VX_DVR_FUSE=0 restores per-frame result slabs + vx::merge_results)"} if fused else
                     {"kernel": "vx::merge_results", "ms_per_launch": round(c.merge_ms / launches, 4),
                      "algorithmic_bytes_per_launch": int(c.pixels / launches * (BYTES_PER_PIXEL_RESULT + BYTES_PER_PIXEL_BLEND / max(fpl, 1))),
                      "note": "reads the per-frame results, applies fragment.frag:158 in frame order, one accumulator "
                              "read + write per launch"} if multi else None,
        }
        out = {
            "metric": "Gsamples/s raymarch @512^3 vol, 1080p; achieved HBM GB/s vs peak, 1/2/4/8 GPU",
            "metric_note": "BASELINE.json's metric string, verbatim.  `value` is the Gsamples/s; the achieved HBM GB/s against the 8 TB/s "
                           "peak is roofline.hbm_measured (rocprofv3 bytes of this command / this run's kernel time) -- the shipped "
                           "kernel takes its taps from LDS windows and is bound by the vector ALUs, so the line's `roofline` is the "
                           "VALU issue roofline (roofline.bound, roofline.frac_kind) and the HBM figure is reported beside it",
            "rehearsal": ("gloo backend, the ranks share one device: a functional rehearsal of the N > 1 path, NOT a "
                          "performance measurement") if rehearse else None,
            "value": round(samples / elapsed / 1e9, 3),
            "value_cold": round(cold_samples / cold["elapsed"] / 1e9, 3) if cold else None,
            "unit": "Gsamples/s",
            "n_gpus": world,
            "steps": a.steps,
            "warmup": a.warmup,
            "ms_per_step": round(elapsed / a.steps * 1e3, 4),
            "ms_per_frame": round(elapsed / frames_timed * 1e3, 4),
            "higher_is_better": True,
            "scaling": "strong",
            "vs_baseline": None,
            "dtype": "f32",
            "data": "synthetic",
            "config": {
                "workload": f"{workload_name(a, world)}: {a.volume}^3 value-noise volume (seed 42), {a.width}x{a.height}, "
                            "DVR trilinear + 128-entry TF LUT (benchmark.json stops), step 0.5 voxel, "
                            "ERT eps 1e-4, clip box (0.25,0,0)-(1,1,0.75), per-frame sub-pixel + start jitter "
                            + ("on" if r.settings.dvr_jitter else "OFF (diagnostic)"),
                "dvr_jitter": bool(r.settings.dvr_jitter),
                "parallelism": (f"image-tiles x{world} (64x64 tiles, "
                                f"{'cost-balanced dealing order' if (world > 1 and not a.no_balance) else 'round-robin'}, volume replicated, RCCL "
                                f"all_gather of the framebuffer every {a.gather_every} frames, overlapped)")
                               if use_dist else "1 GPU",
                "gathers": n_gathers,
                "image_sha256": image_sha,
                "layout": LAYOUT[a.layout],
                "frames_per_step": F, "frames_timed": frames_timed,
                "samples_per_frame": int(samples // frames_timed),
                "frames_per_launch": fpl, "frames_per_launch_requested": P,
                "timed_region_s": round(elapsed, 4),
                "preconditioning": ({**pre, "note": "untimed frames of the same workload before the warm-up steps "
                                     "(--precondition-ms, off by default); value_cold = the same W + K steps measured BEFORE it, "
                                     "on the device as the host-side volume generation left it"} if a.precondition_ms > 0 else None),
                "fixed_overhead_ms": round(fixed_ms, 3) if fixed_ms is not None else None,
                "lane_utilisation": round(c.samples / c.lane_slots, 4) if c.lane_slots else None,
                "device": name, "cus": cus, **info,
            },
            "roofline": roof,
        }
        if world == 1 and not a.no_side_measurements:
            # (1) the same workload with ONE frame per launch (what a host that cannot batch frames gets)
            r.reset_counters()
            n1 = max(8, min(frames_timed, 32))
            run(frames_warm + frames_timed, n1, per_launch=1)
            r.finish()
            c1 = r.counters()
            alg1 = (c1.samples * BYTES_PER_SAMPLE + c1.pixels * BYTES_PER_PIXEL_BLEND) / max(c1.launches, 1)
            k1 = c1.kernel_ms / max(c1.launches, 1) / 1e3
            roof["frames_per_launch_1"] = {
                "frames": int(c1.frames), "launches": int(c1.launches), "avg_kernel_ms": round(k1 * 1e3, 4),
                "gsamples_per_s_kernel_only": round(c1.samples / (c1.kernel_ms / 1e3) / 1e9, 3),
                "achieved": round((c1.samples * NECESSARY_VALU["per_sample"] + c1.tf_samples * NECESSARY_VALU["per_tf_sample"])
                                  / 64.0 / max(c1.launches, 1) / k1 / 1e9, 1),
                "frac": round((c1.samples * NECESSARY_VALU["per_sample"] + c1.tf_samples * NECESSARY_VALU["per_tf_sample"])
                              / 64.0 / max(c1.launches, 1) / k1 / 1e9 / valu_peak, 4),
                "algorithmic_gbs": round(alg1 / k1 / 1e9, 1),
                "algorithmic_model": "16 B/sample + 32 B/pixel/frame (accumulator read + write in the same kernel)"}
            # (2) the limiter the counters name
            if a.layout == 1:
                roof["l1"] = l1_block(r, c)       # the cellquad gather kernel: vector L1 tag pipe
            elif a.layout in (None, 2, 4):
                roof["issue"] = issue_block(r, c, prof_entry)   # the LDS-window kernel: vector-ALU issue
        if world == 1 and not a.no_cpu_baseline:
            out["cpu_baseline"] = cpu_baseline(r, msg)
        else:
            out["cpu_baseline"] = None
        if world == 1 and not a.no_skip_variant:
            # same frames with the exact empty-space skipping switched on (fewer samples are
            # evaluated, so the headline metric above is quoted without it)
            r.settings.dvr_skip_empty = True
            r.bind_uniforms()
            r.render(frames=5, rebind=False); r.finish(); r.reset_counters()
            r.render(frames=P, rebind=False, in_flight=P); r.finish()
            cs_ = r.counters()
            out["config"]["with_empty_space_skipping"] = {
                "ms_per_frame": round(cs_.kernel_ms / cs_.frames, 4),
                "samples_per_frame": int(cs_.samples // cs_.frames),
                "gsamples_per_s": round(cs_.samples / cs_.kernel_ms / 1e6, 1)}
            r.settings.dvr_skip_empty = False
        if world == 1 and not a.no_mode_variants:
            # the other render modes on the same scene (kernel ms per accumulation frame; not the metric)
            other = {}
            for mode, bounces in (("dvr_phong", 1), ("default", 1), ("no_dda", 1), ("raymarch", 1)):
                r.settings.render_mode, r.settings.bounces = mode, bounces
                r.restart_rendering()
                r.bind_uniforms()
                r.render(frames=3, rebind=False); r.finish(); r.reset_counters()
                r.render(frames=P, rebind=False, in_flight=P); r.finish()
                cs_ = r.counters()
                other[mode] = mode_record(mode, cs_, a)
            out["config"]["other_modes"] = other
            out["config"]["other_modes_note"] = (
                "roofline = SURVEY 8(d) byte model / kernel time / 8000 GB/s: 16 B per trilinear sample (default, no_dda), 9 B "
                "per nearest-tap sample (raymarch), 64 B per Phong-shaded DVR sample position (16 B x the sample and its gradient "
                "taps' cells), 4 B per DDA step, 32 B per pixel and frame; lane_utilisation = SQ_ACTIVE_INST_VALU lanes / 64 of "
                "the rocprofv3 PMC pass named in lane_utilisation_source (null when no profile of this build is committed)")
        real_stdout.write(json.dumps(out) + "\n")
        real_stdout.flush()
    if use_dist:
        barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
