#!/usr/bin/env python3
"""Seeded region growing (vx_segment): predicate-pass, flood and statistics times (HIP events, median of repetitions), rounds and
brick visits, beside the host path it replaces -- the densities downloaded (the mask read-back stands in for the bytes) and
scipy.ndimage.label over the same predicate mask on the CPU -- on config 2's bone (256^3 CT phantom), config 3 (512^3 value
noise) at d >= 0.5, a one-voxel serpentine (the worst case for rounds) and a 1024^3 volume (config 3's noise tiled 2 x 2 x 2,
whose densities tile exactly).  Then the host's read-back schedule: the doubling batches capped at VX_SEG_CHECK_MAX = 1, 4, 16,
64 (the default), 256 and 1024 rounds, on the serpentine and config 2's bone.  One JSON line.  Run from the repository root:
python tools/segment_probe.py"""
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

F32 = np.float32


def densities(msg, scale, inv_maj):
    """d over the index extent (Z, Y, X): (scale * v) * inv_maj in fp32, as the device computes it"""
    from oracle import np_oracle as NP
    vol = NP.NpVolume(msg)
    X, Y, Z = (int(e) for e in vol.ext)
    out = np.empty((Z, Y, X), dtype=F32)
    y, x = np.meshgrid(np.arange(Y), np.arange(X), indexing="ij")
    for z in range(Z):
        out[z] = (F32(scale) * vol.brick(x, y, np.full_like(x, z))).astype(F32) * F32(inv_maj)
    return out


def serpentine(X=96, Y=96, Z=24):
    v = np.zeros((Z, Y, X), dtype=np.uint16)
    x = 0
    rows, layers = list(range(0, Y, 2)), list(range(0, Z, 2))
    for li, z in enumerate(layers):
        order = rows if li % 2 == 0 else rows[::-1]
        for ri, y in enumerate(order):
            xe = X - 1 if x == 0 else 0
            v[z, y, min(x, xe):max(x, xe) + 1] = 3000
            x = xe
            if ri + 1 < len(order):
                v[z, (y + order[ri + 1]) // 2, x] = 3000
        if li + 1 < len(layers):
            v[z + 1, order[-1], x] = 3000
    return v, (1.0, 1.0, 1.0)


def renderer(msg):
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer
    r = Volxel3DRenderer(64, 64, device=0)
    r.setup_from_grid(msg)
    r.restore_settings(BENCHMARK_SETTINGS)
    r.settings.render_mode = "dvr"
    return r


def run(name, msg, lo, mask_of, reps, seed=None):
    from scipy import ndimage
    r = renderer(msg)
    try:
        p = r.bind_uniforms()
        host = mask_of(p)                               # the predicate mask the host path labels
        if seed is None:
            z, y, x = np.unravel_index(int(np.argmax(host)), host.shape)
            seed = (int(x), int(y), int(z))
        s = r.segment(seed, lo)                         # warm-up (allocations, code objects)
        ms, wall = [], []
        for _ in range(reps):
            t0 = time.perf_counter()
            s = r.segment(seed, lo)
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(r.segment_stats()[2:])
        t0 = time.perf_counter()
        m = r.segment_mask()
        read_ms = (time.perf_counter() - t0) * 1e3
        t0 = time.perf_counter()
        lab, _ = ndimage.label(host, structure=ndimage.generate_binary_structure(3, 1))
        label_ms = (time.perf_counter() - t0) * 1e3
        same = bool(np.array_equal(m, lab == lab[seed[2], seed[1], seed[0]]))
        nvox = host.size
    finally:
        r.close()
    med = [statistics.median(t[i] for t in ms) for i in range(3)]
    return {"voxels": nvox, "seed": list(seed), "lo": lo, "count": s.count, "rounds": s.rounds, "brick_visits": s.brick_visits,
            "converged": s.converged, "predicate_ms": med[0], "flood_ms": med[1], "stats_ms": med[2],
            "call_ms_median": statistics.median(wall), "mask_readback_ms": read_ms,
            "scipy_label_ms": label_ms, "same_mask_as_scipy": same}


def check_max_sweep(msg, lo, seed, reps):
    """call time and flood time per cap of the read-back batches (VX_SEG_CHECK_MAX is read when a context is created)"""
    row = {}
    for cap in (1, 4, 16, 64, 256, 1024):
        os.environ["VX_SEG_CHECK_MAX"] = str(cap)
        try:
            r = renderer(msg)
        finally:
            del os.environ["VX_SEG_CHECK_MAX"]
        try:
            r.bind_uniforms()
            s = r.segment(seed, lo)
            wall, flood = [], []
            for _ in range(reps):
                t0 = time.perf_counter()
                s = r.segment(seed, lo)
                wall.append((time.perf_counter() - t0) * 1e3)
                flood.append(r.segment_stats()[3])
        finally:
            r.close()
        row[str(cap)] = {"call_ms_median": statistics.median(wall), "flood_ms_median": statistics.median(flood),
                         "rounds": s.rounds, "count": s.count}
    return row


def main(reps=5):
    from volxel_amd import read_u16_stack_to_grid, synth
    out = {}
    msg = read_u16_stack_to_grid(*synth.ct_phantom(256))
    bone = msg
    out["config2_bone"] = run("config2", msg, 0.75, lambda p: densities(msg, p.volume_density_scale, p.volume_inv_maj) >= F32(0.75),
                              reps)
    vox, sp = serpentine()
    msg = read_u16_stack_to_grid(vox, sp)
    out["serpentine_96x96x24"] = run("serpentine", msg, 0.5, lambda p: densities(msg, p.volume_density_scale,
                                                                                 p.volume_inv_maj) >= F32(0.5), reps, seed=(0, 0, 0))
    out["check_max_sweep"] = {"serpentine": check_max_sweep(msg, 0.5, (0, 0, 0), reps),
                              "config2_bone": check_max_sweep(bone, 0.75, tuple(out["config2_bone"]["seed"]), reps)}
    del bone
    vox, sp = synth.value_noise(512, seed=42)
    msg = read_u16_stack_to_grid(vox, sp)
    v512 = densities(msg, 1.0, 1.0)                     # the decoded voxels: (1 * v) * 1 = v

    def mask_from_v(p):
        return ((F32(p.volume_density_scale) * v512).astype(F32) * F32(p.volume_inv_maj)) >= F32(0.5)
    out["config3_512"] = run("config3", msg, 0.5, mask_from_v, reps)
    big = np.tile(vox, (2, 2, 2))
    del vox, msg
    msg = read_u16_stack_to_grid(big, sp)
    del big
    # 512 is a multiple of the brick size: the decoded voxels tile exactly, and d = (scale * v) * inv_maj with this scene's params
    out["tiled_1024"] = run("1024", msg, 0.5, lambda p: np.tile(mask_from_v(p), (2, 2, 2)), max(2, reps // 2))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
