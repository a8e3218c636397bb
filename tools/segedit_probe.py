#!/usr/bin/env python3
"""Segment edits (vx_segment_edit): on config 2's bone (the 256^3 CT phantom at d >= 0.75, the segment of the README's quick
start) the HIP-event time of the edit and of its statistics (median of repetitions) and the kernels launched for dilate 1,
dilate 8, close 3 and fill holes under both connectivities, beside scipy.ndimage's wall time for the same operation on the same
mask on the host, the voxel count before and after, and whether the two masks agree.  A step reads and writes the mask once:
2 * bricks * 64 bytes, printed as step_bytes beside the measured time per step.  One JSON line.  Run from the repository root:
python tools/segedit_probe.py [--n 256] [--reps 5]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=256)
    ap.add_argument("--reps", type=int, default=5)
    a = ap.parse_args()
    from scipy import ndimage
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    msg = read_u16_stack_to_grid(*synth.ct_phantom(a.n))
    r = Volxel3DRenderer(64, 64, device=0)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.render_mode = "dvr"
    # a seed in the spine: the middle of the ellipsoid at (0, 0.35, 0) of the unit cube
    seed = (a.n // 2, int((0.35 + 1.0) / 2.0 * a.n), a.n // 2)
    s0 = r.segment(seed, 0.75)
    m0 = r.segment_mask()
    bricks = int(np.prod([int(e) // 8 for e in msg.index_extent]))
    out = {"n": a.n, "device": r.device_info()[0], "count": s0.count, "bricks": bricks, "step_bytes": 2 * bricks * 64, "cases": []}

    def st(c):
        return ndimage.generate_binary_structure(3, 1 if c == 6 else 3)

    host = {
        "dilate1": lambda c: ndimage.binary_dilation(m0, st(c), iterations=1),
        "dilate8": lambda c: ndimage.binary_dilation(m0, st(c), iterations=8),
        "close3": lambda c: ndimage.binary_erosion(ndimage.binary_dilation(m0, st(c), iterations=3), st(c), iterations=3, border_value=1),
        "fill_holes": lambda c: ndimage.binary_fill_holes(m0, structure=st(c)),
    }
    dev = {"dilate1": ("dilate", 1), "dilate8": ("dilate", 8), "close3": ("close", 3), "fill_holes": ("fill_holes", 1)}
    for name, (op, n) in dev.items():
        for conn in (6, 26):
            edit_ms, stats_ms = [], []
            for _ in range(a.reps):
                r.set_segment_mask(m0)
                s = r.segment_edit(op, steps=n, connectivity=conn)
                launches, e, t = r.segment_edit_stats()
                edit_ms.append(e)
                stats_ms.append(t)
            got = r.segment_mask()
            t0 = time.perf_counter()
            want = host[name](conn)
            host_ms = (time.perf_counter() - t0) * 1e3
            steps = 1 if op == "fill_holes" else (2 * n if op == "close" else n)
            med = statistics.median(edit_ms)
            out["cases"].append({"case": name, "connectivity": conn, "launches": launches, "edit_ms": round(med, 4),
                                 "ms_per_launch": round(med / launches, 4), "stats_ms": round(statistics.median(stats_ms), 4),
                                 "scipy_ms": round(host_ms, 1), "count_after": s.count, "rounds": s.rounds,
                                 "equal": bool(np.array_equal(got, want)),
                                 "GBps": None if op == "fill_holes" else round(steps * 2 * bricks * 64 / (med * 1e-3) / 1e9, 1)})
    r.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
