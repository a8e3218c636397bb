#!/usr/bin/env python3
"""Intensity projections (VX_MODE_MIP / VX_MODE_MINIP) against DVR at 1920x1080: kernel time per frame at 32 frames per launch
and at 1, with samples and skip_steps per frame, on two scenes -- BASELINE config 3 (512^3 value noise, clip box, jitter:
bench.py build_scene) and config 2 (256^3 CT phantom, whole volume, where range skipping should pay).  Runs: DVR, MIP with
skipping off and on, MinIP with skipping on, and generic MIP (VX_DVR_KERNEL=generic, in a child process).  One JSON line.
Run from the repository root: python tools/projection_probe.py"""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

RUNS = {"dvr": ("dvr", False), "mip_skip_off": ("mip", False), "mip_skip_on": ("mip", True), "minip_skip_on": ("minip", True)}


def scene(name):
    if name == "config3":
        r, _, _ = bench.build_scene(1920, 1080, 512, 0, 1, 0)
        return r
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    msg = read_u16_stack_to_grid(*synth.ct_phantom(256))
    r = Volxel3DRenderer(1920, 1080, device=0)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    s = r.settings
    s.volume_clip_min, s.volume_clip_max = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    s.dvr_step_voxels, s.dvr_ert_epsilon, s.dvr_jitter, s.max_samples = 0.5, 1e-4, True, 1 << 30
    return r


def measure(r, frames, in_flight, reps):
    r.restart_rendering()
    r.render(frames=frames, in_flight=in_flight)      # warm-up (and the bound table, if it is stale)
    r.finish()
    r.reset_counters()
    for _ in range(reps):
        r.render(frames=frames, in_flight=in_flight)
    r.finish()
    c = r.counters()
    return {"ms": round((c.kernel_ms + c.merge_ms) / c.frames, 4), "samples": c.samples // c.frames,
            "skip_steps": c.skip_steps // c.frames}


def run(name, runs):
    r = scene(name)
    out = {}
    for key in runs:
        mode, skip = RUNS[key]
        r.settings.render_mode, r.settings.dvr_skip_empty = mode, skip
        out[key] = {"fpl32": measure(r, 32, 32, 8), "fpl1": measure(r, 8, 1, 4)}
    r.close()
    return out


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--child":     # generic MIP: VX_DVR_KERNEL is read when the context is created
        print(json.dumps(run(sys.argv[2], ["mip_skip_off"])["mip_skip_off"]), flush=True)
        return
    out = {}
    for name in ("config3", "config2"):
        out[name] = run(name, list(RUNS))
        env = dict(os.environ, VX_DVR_KERNEL="generic")
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", name], env=env, cwd=ROOT,
                               capture_output=True, text=True, check=True)
        out[name]["generic_mip"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
