#!/usr/bin/env python3
"""The GPU mesher (vx_mesh_extract): config 2's bone (iso = 0.75 on the 256^3 CT phantom) as a density mesh and as the mesh of
its segment, config 3's volume (value noise 512^3 at its median positive density), and a 1024^3 CT phantom when the device
holds it.  Per case: vertices, triangles, cell blocks and active ones, kernels launched, the HIP-event time of each stage
(inside words | active cells and scan | emission; median of repetitions), vertices and triangles per second of kernel time, the
read-back time (vx_mesh_read into host arrays, wall clock), and for the 256^3 cases the wall time of the NumPy restatement
(tests/mesh_ref.py) on the same input and whether the two meshes agree after the canonical sort.  One JSON line.  Run from the
repository root: python tools/mesh_probe.py [--reps 5] [--big 1024] (--big 0: without the large volume)"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def run(r, reps, **kw):
    ms, read_ms = [], []
    for _ in range(reps):
        t0 = time.perf_counter()
        m = r.extract_mesh(space="voxel", **kw)
        wall = (time.perf_counter() - t0) * 1e3
        launches, a, b, c = r.mesh_stats()
        ms.append((a, b, c))
        read_ms.append(wall - (a + b + c))
    res = r.last_mesh_result
    med = [statistics.median(x[i] for x in ms) for i in range(3)]
    total = sum(med)
    return m, {"vertices": int(res.vertices), "triangles": int(res.triangles), "blocks": int(res.blocks),
               "active_blocks": int(res.active_blocks), "launches": launches, "inside_ms": round(med[0], 4),
               "active_scan_ms": round(med[1], 4), "emit_ms": round(med[2], 4), "kernel_ms": round(total, 4),
               "Mvertices_per_s": round(int(res.vertices) / (total * 1e-3) / 1e6, 1) if total > 0 else None,
               "Mtriangles_per_s": round(int(res.triangles) / (total * 1e-3) / 1e6, 1) if total > 0 else None,
               "host_side_ms": round(statistics.median(read_ms), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--big", type=int, default=1024)
    a = ap.parse_args()
    from tests import mesh_ref as MR
    from tests import segment_ref as SG
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    out = {"cases": []}

    def renderer(msg):
        r = Volxel3DRenderer(64, 64, device=0)
        r.setup_from_grid(msg)
        r.restore_settings(BENCHMARK_SETTINGS)
        r.settings.render_mode = "dvr"
        return r

    def same(m, want):
        g, w = MR.canonical(m.vertices.astype(np.float32), m.cells, m.triangles), MR.canonical(*want)
        return bool(all(x.shape == y.shape and np.array_equal(x.view(np.uint32), y.view(np.uint32)) for x, y in zip(g, w)))

    # config 2: the 256^3 CT phantom, bone
    n = 256
    msg = read_u16_stack_to_grid(*synth.ct_phantom(n))
    r = renderer(msg)
    out["device"] = r.device_info()[0]
    p = r.bind_uniforms()
    d = SG.densities(msg, p.volume_density_scale, p.volume_inv_maj)
    m, row = run(r, a.reps, iso=0.75)
    t0 = time.perf_counter()
    want = MR.extract_density(d, 0.75)
    row.update(case="phantom256_bone_density", numpy_ms=round((time.perf_counter() - t0) * 1e3, 1), equal=same(m, want))
    out["cases"].append(row)
    seed = (n // 2, int((0.35 + 1.0) / 2.0 * n), n // 2)
    s = r.segment(seed, 0.75)
    r.segment_edit("close", steps=2, connectivity=6)
    mask = r.segment_mask()
    m, row = run(r, a.reps, segment=True)
    t0 = time.perf_counter()
    want = MR.extract_segment(mask)
    row.update(case="phantom256_bone_segment_closed2", numpy_ms=round((time.perf_counter() - t0) * 1e3, 1), equal=same(m, want),
               segment_voxels=int(mask.sum()))
    out["cases"].append(row)
    r.close()
    # config 3: bench.py's 512^3 scene at iso = 0.5 (tools/iso_probe.py's surface); then the large phantom
    import bench
    print("building config 3 ...", file=sys.stderr, flush=True)
    r, _, _ = bench.build_scene(64, 64, 512, 0, 1, 0)
    m, row = run(r, a.reps, iso=0.5)
    row.update(case="config3_512", iso=0.5)
    out["cases"].append(row)
    r.close()
    if a.big:
        print(f"building the {a.big}^3 phantom ...", file=sys.stderr, flush=True)
        try:
            r = renderer(read_u16_stack_to_grid(*synth.ct_phantom(a.big)))
            m, row = run(r, a.reps, iso=0.75)
            row.update(case=f"phantom{a.big}_bone", iso=0.75)
            r.close()
        except (MemoryError, RuntimeError) as e:   # the device or the host does not hold it
            row = {"case": f"phantom{a.big}_bone", "skipped": str(e)[:200]}
        out["cases"].append(row)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
