#!/usr/bin/env python3
"""First-hit isosurfaces (vx_isosurface) at 1920x1080, refine 8: kernel time (HIP events, median of repetitions) with range
skipping off and on, with hits, march samples and samples passed over, on config 2 (256^3 CT phantom, whole volume) at a bone
threshold and on config 3 (512^3 value noise, bench.py build_scene) at a mid threshold; a lone DVR frame of each scene beside
them for scale.  One JSON line.  Run from the repository root: python tools/iso_probe.py"""
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def scene(name):
    if name == "config3":
        r, _, _ = bench.build_scene(1920, 1080, 512, 0, 1, 0)
        return r, 0.5
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    msg = read_u16_stack_to_grid(*synth.ct_phantom(256))
    r = Volxel3DRenderer(1920, 1080, device=0)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    s = r.settings
    s.volume_clip_min, s.volume_clip_max = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    s.dvr_step_voxels, s.dvr_jitter = 0.5, False
    return r, 0.75


def main(reps=20):
    out = {}
    for name in ("config2", "config3"):
        r, iso = scene(name)
        try:
            row = {"iso": iso}
            for skip in (False, True):
                r.isosurface(iso, refine=8, skip=skip)       # warm-up (and the bound table)
                ms = []
                for _ in range(reps):
                    r.isosurface(iso, refine=8, skip=skip)
                    ms.append(r.iso_stats()[5])
                rays, hits, samples, refine, skipped, _ = r.iso_stats()
                row["skip_on" if skip else "skip_off"] = {"kernel_ms_median": statistics.median(ms), "kernel_ms_min": min(ms),
                                                          "rays": rays, "hits": hits, "samples": samples,
                                                          "refine_samples": refine, "skipped": skipped}
            r.settings.render_mode = "dvr"
            r.restart_rendering()
            r.render(frames=1, in_flight=1)
            r.finish()
            ms = []
            for _ in range(reps):
                r.reset_counters()
                r.render(frames=1, in_flight=1)
                r.finish()
                ms.append(r.counters().last_kernel_ms)
            row["dvr_frame_kernel_ms_median"] = statistics.median(ms)
            out[name] = row
        finally:
            r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
