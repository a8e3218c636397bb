#!/usr/bin/env python3
"""Distances and margins (vx_segment_distance, vx_segment_margin): on config 2's bone (the 256^3 CT phantom at d >= 0.75) and on
config 3 at d >= 0.5 (512^3 value noise) the HIP-event times of the x, y and z pass and of the compare / reduction
(vx_distance_stats; median, min and max over warm repetitions) for a 5 mm grow, a 3 mm close and the uncapped field at the
volume's own spacing -- beside scipy.ndimage.distance_transform_edt on the host for the same mask (wall time, and how many
voxels of its ball differ: ties at the radius round differently in float64) and beside segment_edit("dilate", n, 26) for the n
that reaches the same in-plane radius, the nearest thing the voxel edits offer.  One JSON line.  Run from the repository root:
python tools/distance_probe.py [--reps 7] [--skip-512] [--skip-scipy]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def passes(samples):
    """samples: distance_stats() tuples -> per-pass spread and the spread of their sum"""
    cols = list(zip(*[s[1:] for s in samples]))
    out = {k: spread(c) for k, c in zip(("x_ms", "y_ms", "z_ms", "compare_ms"), cols)}
    out["total_ms"] = spread([sum(s[1:]) for s in samples])
    out["launches"] = samples[0][0]
    return out


def run(r, m0, reps, scipy_too):
    from volxel_amd import _checks
    spacing = _checks.spacing(None, r.volume.grid.transform)
    out = {"spacing": spacing, "count": int(m0.sum()), "voxels": int(m0.size)}
    edt = None
    if scipy_too:
        from scipy import ndimage
        t0 = time.perf_counter()
        edt = ndimage.distance_transform_edt(~m0, sampling=spacing[::-1])
        out["scipy_edt_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
        print(f"scipy edt {out['scipy_edt_ms']} ms", file=sys.stderr, flush=True)
    # the uncapped field
    samples = []
    for i in range(reps + 1):
        d = r.segment_distance()
        if i:
            samples.append(r.distance_stats())
    out["field_uncapped"] = passes(samples)
    out["field_uncapped"]["max_distance"] = d.max_distance
    if edt is not None:
        f = np.sqrt(d.squared().astype(np.float64))
        out["field_uncapped"]["max_rel_diff_vs_scipy"] = float((np.abs(f - edt)[edt > 0] / edt[edt > 0]).max())
    for name, op, radius in (("grow_5mm", "grow", 5.0), ("close_3mm", "close", 3.0)):
        samples = []
        for i in range(reps + 1):
            r.set_segment_mask(m0)
            s = r.segment_margin(op, radius)
            if i:
                samples.append(r.distance_stats())
        case = passes(samples)
        case["count_after"] = s.count
        got = r.segment_mask()
        if edt is not None:
            from scipy import ndimage
            t0 = time.perf_counter()
            want = edt <= radius
            if op == "close":
                want = want & ~(ndimage.distance_transform_edt(want, sampling=spacing[::-1]) <= radius)
            case["scipy_ms"] = round((time.perf_counter() - t0) * 1e3 + out["scipy_edt_ms"], 1)
            case["differs_from_scipy"] = int((got ^ want).sum())
            print(f"{name}: scipy {case['scipy_ms']} ms", file=sys.stderr, flush=True)
        # the voxel edit that reaches the same in-plane radius
        n = min(int(np.ceil(radius / min(spacing[0], spacing[1]))), 1024)
        edit = []
        for i in range(reps + 1):
            r.set_segment_mask(m0)
            e = r.segment_edit("dilate" if op == "grow" else "close", steps=n, connectivity=26)
            if i:
                edit.append(r.segment_edit_stats()[1])
        case["voxel_edit"] = {"op": "dilate" if op == "grow" else "close", "steps": n, "connectivity": 26, "edit_ms": spread(edit),
                              "count_after": e.count}
        out[name] = case
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--skip-scipy", action="store_true")
    a = ap.parse_args()
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    out = {}
    for key, n in (("config2_bone_256", 256), ("config3_512", 512)):
        if n == 512 and a.skip_512:
            continue
        vox, sp = synth.ct_phantom(n) if n == 256 else synth.value_noise(512, seed=42)
        r = Volxel3DRenderer(64, 64, device=0)
        r.setup_from_grid(read_u16_stack_to_grid(vox, sp))
        r.restore_settings(BENCHMARK_SETTINGS)
        r.settings.render_mode = "dvr"
        if n == 256:
            r.segment((n // 2, int((0.35 + 1.0) / 2.0 * n), n // 2), 0.75)      # a seed in the spine, as tools/segedit_probe.py
        else:
            r.threshold(0.5)
        out["device"] = r.device_info()[0]
        out[key] = run(r, r.segment_mask(), a.reps, not a.skip_scipy)
        r.close()
        print(f"{key} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
