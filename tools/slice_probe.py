#!/usr/bin/env python3
"""Slices (vx_slice) on the config-3 value noise: ms per slice, Gsamples/s and the bytes a slice has to read, for
  axial512    a 512^2 axial slice of the 512^3 volume (one sample per pixel)
  mip64_512   a 1024^2 oblique 64-sample MIP slab of the 512^3 volume
  mip64_1024  the same slab on the 1024^3 volume (--no-1024 skips it)
Each figure is the mean of the HIP-event kernel times of `--reps` slices after `--warmup` (no outputs copied: vx_slice with both
pointers NULL), repeated `--runs` times; `spread` is the smallest and largest run mean.  `read_bytes` counts the distinct 8^3
bricks of the brickf32 layout that hold a tap of some sample, at 2 KiB each (a lower bound on what the gathers fetch from
HBM), and `hbm_floor_us` is that plus the W*H*4 bytes of values written at 6.29 TB/s (a float4 copy on this device).
One JSON line.  Run from the repository root: python tools/slice_probe.py"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402

HBM_BPS = 6.29e12


def oblique_slab(r):
    from volxel_amd import oblique
    # the plane through the centre of the volume, tilted about two axes; 1024 pixels of 1/1024 world units (the volume's
    # longest side is 1); 64 samples over 0.06 world units (31 voxels of the 512^3 volume)
    return oblique(r, center=(0.0, 0.0, 0.0), normal=(0.3, -0.5, 0.8), up=(0.1, 1.0, 0.2), pixel_size=1.0 / 1024,
                   size=(1024, 1024), thickness=0.06, samples=64)


def read_bytes(sp, extent):
    """2 KiB x the distinct 8^3 bricks holding a tap (voxels i, i + 1 per axis of the cell of a sample position)"""
    bc = [(int(e) + 7) // 8 for e in extent]
    seen = np.zeros(bc[0] * bc[1] * bc[2], dtype=bool)
    W, H = int(sp.size[0]), int(sp.size[1])
    x, y = np.meshgrid(np.arange(W, dtype=np.float32), np.arange(H, dtype=np.float32))
    o, du, dv, dn = [np.asarray(getattr(sp, n)[:], dtype=np.float32) for n in ("origin", "du", "dv", "dn")]
    base = [o[a] + x * du[a] + y * dv[a] for a in range(3)]
    for s in range(int(sp.slab_samples)):
        cell = [np.floor(base[a] + np.float32(s) * dn[a]).astype(np.int64) for a in range(3)]
        for dz in (0, 1):
            for dy in (0, 1):
                for dx in (0, 1):
                    i = [cell[0] + dx, cell[1] + dy, cell[2] + dz]
                    ok = np.ones(i[0].shape, dtype=bool)
                    for a in range(3):
                        ok &= (i[a] >= 0) & (i[a] < extent[a])
                    b = ((i[2][ok] >> 3) * bc[1] + (i[1][ok] >> 3)) * bc[0] + (i[0][ok] >> 3)
                    seen[b] = True
    return int(seen.sum()) * 2048


def measure(r, sp, reduce, warmup, reps, runs):
    from volxel_amd import _abi
    q = _abi.VxSliceParams.from_buffer_copy(sp)
    q.reduce = _abi.SLICE_REDUCE[reduce]
    r.bind_uniforms()
    lib, ctx = r._lib, r._ctx
    for _ in range(warmup):
        r._check(lib.vx_slice(ctx, C.byref(q), None, None))
    means = []
    for _ in range(runs):
        t = 0.0
        for _ in range(reps):
            r._check(lib.vx_slice(ctx, C.byref(q), None, None))
            t += r.slice_stats()[1]
        means.append(t / reps)
    n = r.slice_stats()[0]
    ms = float(np.mean(means))
    rb = read_bytes(q, [int(e) for e in r.volume.grid.index_extent])
    wb = int(q.size[0]) * int(q.size[1]) * 4
    return {"ms": round(ms, 4), "spread_ms": [round(min(means), 4), round(max(means), 4)], "samples": n,
            "gsamples_per_s": round(n / (ms * 1e-3) / 1e9, 2), "read_bytes": rb, "written_bytes": wb,
            "hbm_floor_us": round((rb + wb) / HBM_BPS * 1e6, 2), "reps": reps, "runs": runs}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--no-1024", action="store_true")
    ap.add_argument("--out", default=None, help="also write the JSON here")
    a = ap.parse_args()
    from volxel_amd import axial
    out = {}
    r, _, _ = bench.build_scene(256, 256, 512, 0, 1, 0)
    out["axial512"] = measure(r, axial(r, 256), "mean", a.warmup, a.reps, a.runs)
    out["mip64_512"] = measure(r, oblique_slab(r), "max", a.warmup, a.reps, a.runs)
    out["device"] = r.device_info()[0]
    r.close()
    if not a.no_1024:
        r, _, _ = bench.build_scene(256, 256, 1024, 0, 1, 0)
        out["mip64_1024"] = measure(r, oblique_slab(r), "max", a.warmup, a.reps, a.runs)
        r.close()
    line = json.dumps(out)
    print(line, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
