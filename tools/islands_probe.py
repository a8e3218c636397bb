#!/usr/bin/env python3
"""Islands (vx_segment_threshold, vx_segment_islands): the times of the labelling passes (HIP events; the host's ranking of the
table in wall clock), median of repetitions after a warm-up, and each modifying op end to end, beside the host path they
replace -- scipy.ndimage.label + np.bincount of the same mask on the CPU, with the mask read-back and re-upload that path also
needs listed on their own -- on config 2's bone (256^3 CT phantom), config 3 (512^3 value noise) at d >= 0.5, the one-voxel
serpentine next to the flood of segment() over it, and (--with-1024) config 3's noise tiled 2 x 2 x 2.  One JSON line.  Run from
the repository root: python tools/islands_probe.py"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

from segment_probe import F32, densities, renderer, serpentine  # noqa: E402

PASSES = ("local_ms", "merge_ms", "flatten_ms", "table_ms", "host_rank_ms", "apply_ms", "stats_ms")


def timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, (time.perf_counter() - t0) * 1e3


def run(msg, lo, mask_of, reps, conn=6, flood_seed=None):
    from scipy import ndimage
    r = renderer(msg)
    try:
        p = r.bind_uniforms()
        host = mask_of(p)
        row = {"voxels": int(host.size), "lo": lo, "connectivity": conn}
        s, row["threshold_call_ms"] = timed(lambda: r.threshold(lo))
        s, row["threshold_call_ms"] = timed(lambda: r.threshold(lo))
        row["count"] = s.count
        r.islands(conn)                                  # warm-up (allocations, code objects)
        wall, passes = [], []
        for _ in range(reps):
            isl, ms = timed(lambda: r.islands(conn))
            wall.append(ms)
            passes.append(r.islands_stats())
        row["islands"], row["largest"], row["launches"] = isl.count, isl.largest, passes[0][0]
        row["label_call_ms"] = statistics.median(wall)
        for i, name in enumerate(PASSES):
            row[name] = statistics.median(t[1 + i] for t in passes)
        row["label_and_table_kernels_ms"] = sum(row[n] for n in PASSES[:4])
        _, row["labels_readback_ms"] = timed(isl.labels)
        m, row["mask_readback_ms"] = timed(r.segment_mask)
        _, row["mask_upload_ms"] = timed(lambda: r.set_segment_mask(m))
        anchor = isl.table[0]["anchor"] if isl.count else (0, 0, 0)
        for name, call in (("keep_largest_1", lambda: r.keep_largest_islands(1, conn)),
                           ("remove_small_10", lambda: r.remove_small_islands(10, conn)),
                           ("keep_at_anchor0", lambda: r.keep_island_at(anchor, conn))):
            ts = []
            for _ in range(reps):
                r.threshold(lo)
                s, ms = timed(call)
                ts.append(ms)
            row[name + "_call_ms"] = statistics.median(ts)
            row[name + "_kept"] = s.kept
        if flood_seed is not None:                       # the flood by rounds over the same mask
            r.segment(flood_seed, lo, connectivity=conn)
            ts = []
            for _ in range(reps):
                s, ms = timed(lambda: r.segment(flood_seed, lo, connectivity=conn))
                ts.append(ms)
            row["flood_call_ms"], row["flood_rounds"], row["flood_ms"] = statistics.median(ts), s.rounds, r.segment_stats()[3]

        def scipy_path():
            lab, n = ndimage.label(host, structure=ndimage.generate_binary_structure(3, 1 if conn == 6 else 3))
            return n, np.bincount(lab.ravel())
        (n, counts), row["scipy_label_bincount_ms"] = timed(scipy_path)
        row["same_as_scipy"] = bool(n == isl.count and np.array_equal(m, host) and
                                    np.array_equal(np.sort(counts[1:])[::-1].astype(np.uint64), isl.sizes))
    finally:
        r.close()
    return row


def main(reps=5):
    from volxel_amd import read_u16_stack_to_grid, synth
    out = {}
    msg = read_u16_stack_to_grid(*synth.ct_phantom(256))
    out["config2_bone"] = run(msg, 0.75, lambda p: densities(msg, p.volume_density_scale, p.volume_inv_maj) >= F32(0.75), reps)
    vox, sp = serpentine()
    msg = read_u16_stack_to_grid(vox, sp)
    out["serpentine_96x96x24"] = run(msg, 0.5, lambda p: densities(msg, p.volume_density_scale, p.volume_inv_maj) >= F32(0.5), reps,
                                     flood_seed=(0, 0, 0))
    vox, sp = synth.value_noise(512, seed=42)
    msg = read_u16_stack_to_grid(vox, sp)
    v512 = densities(msg, 1.0, 1.0)

    def mask_from_v(p):
        return ((F32(p.volume_density_scale) * v512).astype(F32) * F32(p.volume_inv_maj)) >= F32(0.5)
    out["config3_512"] = run(msg, 0.5, mask_from_v, reps)
    if "--with-1024" in sys.argv:
        big = np.tile(vox, (2, 2, 2))
        del vox, msg
        msg = read_u16_stack_to_grid(big, sp)
        del big
        out["tiled_1024"] = run(msg, 0.5, lambda p: np.tile(mask_from_v(p), (2, 2, 2)), max(2, reps // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
