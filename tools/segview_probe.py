#!/usr/bin/env python3
"""Segment views (vx_set_segment_view): the cost of the masked kernels on BASELINE config 3 (512^3 value noise, clip box, jitter:
bench.py build_scene) at 1920x1080.  The segment is the 6-connected component of d >= 0.5 holding the densest voxel (as
tools/segment_probe.py).  Kernel time per frame at 32 frames per launch for DVR and MIP with the view OFF -- range skipping off
(the SKIP = false instance every masked launch runs) and on -- ONLY and HIDE; then the isosurface at 1080p (iso 0.5, refine 8):
kernel time, median of 5 calls, OFF with and without skipping, ONLY and HIDE.  One JSON line.  Run from the repository root:
python tools/segview_probe.py"""
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

F32 = np.float32


def measure(r, frames=32, in_flight=32, reps=8):
    r.restart_rendering()
    r.render(frames=frames, in_flight=in_flight)      # warm-up (and any table that is stale)
    r.finish()
    r.reset_counters()
    for _ in range(reps):
        r.render(frames=frames, in_flight=in_flight)
    r.finish()
    c = r.counters()
    return {"ms": round((c.kernel_ms + c.merge_ms) / c.frames, 4), "samples": c.samples // c.frames}


def iso(r, skip, reps=5):
    r.isosurface(0.5, skip=skip)
    ms = []
    for _ in range(reps):
        r.isosurface(0.5, skip=skip)
        ms.append(r.iso_stats()[5])
    st = r.iso_stats()
    return {"ms": round(statistics.median(ms), 4), "hits": st[1], "samples": st[2], "skipped": st[4]}


def main():
    r, msg, _ = bench.build_scene(1920, 1080, 512, 0, 1, 0)
    out = {}
    try:
        p = r.bind_uniforms()
        from oracle import np_oracle as NP
        vol = NP.NpVolume(msg)
        X, Y, Z = (int(e) for e in vol.ext)
        y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
        best, seed = -1.0, (0, 0, 0)
        for z in range(0, Z, 8):   # the densest voxel of every 8th slice: a seed inside a large component
            d = (F32(p.volume_density_scale) * vol.brick(x, y, np.full_like(x, z))).astype(F32) * F32(p.volume_inv_maj)
            i = int(np.argmax(d))
            if d.flat[i] > best:
                best, seed = float(d.flat[i]), (int(i % X), int(i // X), z)
        s = r.segment(seed, 0.5)
        out["segment"] = {"seed": list(seed), "count": s.count, "voxels": X * Y * Z}
        for mode in ("dvr", "mip"):
            r.settings.render_mode = mode
            row = {}
            for view, skip in (("off", False), ("off", True), ("only", False), ("hide", False)):
                r.settings.dvr_skip_empty = skip
                r.segment_view = view
                row[view if view != "off" else ("off_skip" if skip else "off_noskip")] = measure(r)
            r.segment_view = "off"
            out[mode + "_fpl32"] = row
        r.settings.render_mode = "dvr"
        row = {}
        for view, skip in (("off", False), ("off", True), ("only", False), ("hide", False)):
            r.segment_view = view
            row[view if view != "off" else ("off_skip" if skip else "off_noskip")] = iso(r, skip)
        out["iso_1080p"] = row
    finally:
        r.close()
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
