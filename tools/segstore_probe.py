#!/usr/bin/env python3
"""The segment store (vx_segment_store .. vx_segments_labelmap): on config 2's bone (the 256^3 CT phantom at d >= 0.75) and on
config 3 at d >= 0.5 (512^3 value noise), with A the mask and B the mask grown by 2 mm in two slots, over warm repetitions:

  combine    the HIP-event time of the word-wise kernel and of the statistics behind it (vx_segment_edit_stats) and the wall time
             of the whole call, for subtract, union and invert of B against A; the bytes the kernel moves (two masks read, one
             written: 3 x 1 bit per voxel; invert: 2 x) over its time, beside the 8 TB/s HBM peak; beside the wall time of the host route to the
             same mask, segment_mask() + NumPy + set_segment_mask() with the slot's mask on the host already
  compare    the wall time of the whole call without and with the Hausdorff distances, and with them the HIP-event times of the
             two transforms and their reductions (vx_distance_stats; the popcount and label-map kernels carry no event timer:
             a kernel trace of this probe, one volume at a time with --skip-256 / --skip-512, gives their times); beside
             segment_mask() + NumPy for the counts and + two scipy.ndimage.distance_transform_edt for the distances, with the
             largest relative difference of the two results
  label map  the wall time of the whole call (kernel, and the copy of 1 B per voxel to the host, which dominates), beside two
             load_segment() + segment_mask() read-backs and np.where on the host

One JSON line.  Run from the repository root: python tools/segstore_probe.py [--reps 7] [--skip-256] [--skip-512] [--skip-scipy]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12     # bytes per second, MI355X


def spread(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def wall_ms(f):
    t0 = time.perf_counter()
    out = f()
    return (time.perf_counter() - t0) * 1e3, out


def run(r, reps, scipy_too):
    from volxel_amd import _checks
    spacing = _checks.spacing(None, r.volume.grid.transform)
    A = r.segment_mask()
    r.store_segment(0)
    r.segment_margin("grow", 2.0)
    B = r.segment_mask()
    r.store_segment(1)
    out = {"spacing": spacing, "voxels": int(A.size), "count_a": int(A.sum()), "count_b": int(B.sum()), "slot_bytes": int(A.size // 8)}
    # ---- combine
    # (the current segment is B, the slot A: subtract leaves the 2 mm shell, union B itself, invert everything but B)
    for op, host in (("subtract", lambda b: b & ~A), ("union", lambda b: b | A), ("invert", lambda b: ~b)):
        kernel, stats, call, route = [], [], [], []
        for i in range(reps + 1):
            r.load_segment(1)
            ms, seg = wall_ms(lambda: r.segment_combine(op) if op == "invert" else r.segment_combine(op, 0))
            st = r.segment_edit_stats()
            r.load_segment(1)
            hms, hseg = wall_ms(lambda: r.set_segment_mask(host(r.segment_mask())))
            assert hseg.count == seg.count
            if i:
                kernel.append(st[1]), stats.append(st[2]), call.append(ms), route.append(hms)
        moved = (2 if op == "invert" else 3) * (A.size // 8)
        k = statistics.median(kernel)
        out[f"combine_{op}"] = {"kernel_ms": spread(kernel), "stats_ms": spread(stats), "call_ms": spread(call), "count_after": seg.count,
                                "bytes_moved": moved, "kernel_gbs": round(moved / (k * 1e-3) / 1e9, 1),
                                "hbm_peak_fraction": round(moved / (k * 1e-3) / HBM_PEAK, 4), "host_route_ms": spread(route)}
    # ---- compare
    r.load_segment(0)
    quick, full, passes, host_counts = [], [], [], []
    for i in range(reps + 1):
        qms, q = wall_ms(lambda: r.segment_compare(1, hausdorff=False))
        fms, c = wall_ms(lambda: r.segment_compare(1))
        st = r.distance_stats()
        hms, hc = wall_ms(lambda: (lambda a: (int(a.sum()), int(B.sum()), int((a & B).sum())))(r.segment_mask()))
        assert hc == (q.count_a, q.count_b, q.count_and) == (c.count_a, c.count_b, c.count_and)
        if i:
            quick.append(qms), full.append(fms), passes.append(st), host_counts.append(hms)
    cols = list(zip(*[s[1:] for s in passes]))
    out["compare_counts"] = {"call_ms": spread(quick), "dice": q.dice, "jaccard": q.jaccard, "host_route_ms": spread(host_counts)}
    out["compare_hausdorff"] = {"call_ms": spread(full), "launches": passes[0][0], "hausdorff_ab": c.hausdorff_ab,
                                "hausdorff_ba": c.hausdorff_ba, "argmax_ab": c.argmax_ab, "argmax_ba": c.argmax_ba,
                                "kernel_ms": spread([sum(s[1:]) for s in passes]),
                                **{k: spread(v) for k, v in zip(("x_ms", "y_ms", "z_ms", "reduce_ms"), cols)}}
    if scipy_too:
        from scipy import ndimage

        def host_hausdorff():
            a = r.segment_mask()
            to_b = ndimage.distance_transform_edt(~B, sampling=spacing[::-1])
            to_a = ndimage.distance_transform_edt(~a, sampling=spacing[::-1])
            return float(to_b[a].max()), float(to_a[B].max())
        hms, (hab, hba) = wall_ms(host_hausdorff)
        out["compare_hausdorff"]["scipy_ms"] = round(hms, 1)
        out["compare_hausdorff"]["max_rel_diff_vs_scipy"] = max(abs(c.hausdorff_ab - hab) / hab if hab else 0.0,
                                                                 abs(c.hausdorff_ba - hba) / hba if hba else 0.0)
        print(f"scipy hausdorff {hms:.0f} ms", file=sys.stderr, flush=True)
    # ---- label map
    call, route = [], []
    for i in range(reps + 1):
        ms, (labels, overlaps) = wall_ms(lambda: r.segments_labelmap([0, 1]))

        def host_labels():
            m = []
            for k in (0, 1):
                r.load_segment(k)
                m.append(r.segment_mask())
            return np.where(m[0], 1, np.where(m[1], 2, 0)).astype(np.uint8), int((m[0] & m[1]).sum())
        hms, (hl, ho) = wall_ms(host_labels)
        assert ho == overlaps and np.array_equal(hl, labels)
        if i:
            call.append(ms), route.append(hms)
    out["labelmap"] = {"call_ms": spread(call), "bytes_to_host": int(labels.size), "overlaps": overlaps, "host_route_ms": spread(route)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-256", action="store_true")
    ap.add_argument("--skip-512", action="store_true")
    ap.add_argument("--skip-scipy", action="store_true")
    a = ap.parse_args()
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    out = {}
    for key, n in (("config2_bone_256", 256), ("config3_512", 512)):
        if (n == 512 and a.skip_512) or (n == 256 and a.skip_256):
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
        out[key] = run(r, a.reps, not a.skip_scipy)
        r.close()
        print(f"{key} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
