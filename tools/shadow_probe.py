#!/usr/bin/env python3
"""Shadowed DVR on BASELINE config 3 (512^3 value noise, 1920x1080, clip box, ERT, jitter -- bench.py build_scene): the
light-grid build per stride (HIP-event time, light-march samples, grid memory) and the kernel time per frame with and
without shadows at 32 frames per launch and at 1, both under the directional light (use_env off).  One JSON line.  Run from the repository root: python tools/shadow_probe.py"""
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402


def ms_per_frame(r, frames, in_flight, reps):
    r.restart_rendering()
    r.render(frames=frames, in_flight=in_flight)      # warm-up (and the light grid, if it is stale)
    r.finish()
    r.reset_counters()
    for _ in range(reps):
        r.render(frames=frames, in_flight=in_flight)
    r.finish()
    c = r.counters()
    return (c.kernel_ms + c.merge_ms) / c.frames


def main():
    r, msg, info = bench.build_scene(1920, 1080, 512, 0, 1, 0)
    r.settings.use_env = False      # shadows need the directional light (both sides of the A/B run without the map)
    out = {"builds": {}, "ms_per_frame": {}}
    for s in (1, 2, 4):
        r.settings.dvr_shadow_stride = s
        r.restart_rendering()
        r.render(frames=1, in_flight=1)
        r.finish()
        b, n, ms = r.shadow_stats()
        nx, ny, nz = [(e - 1 + s - 1) // s + 1 for e in msg.index_extent]
        out["builds"][s] = {"build_ms": round(ms, 3), "light_samples": n, "nodes": nx * ny * nz,
                            "grid_mb": round(4 * nx * ny * nz / 1e6, 1), "gsamples_per_s": round(n / ms / 1e6, 1)}
    for s in (0, 2):
        r.settings.dvr_shadow_stride = s
        out["ms_per_frame"][f"stride{s}_fpl32"] = round(ms_per_frame(r, 32, 32, 8), 4)
        out["ms_per_frame"][f"stride{s}_fpl1"] = round(ms_per_frame(r, 8, 1, 4), 4)
    print(json.dumps(out), flush=True)
    r.close()


if __name__ == "__main__":
    main()
