#!/usr/bin/env python3
"""The histograms (vx_histogram): on config 2 (the 256^3 CT phantom; the bone is the segment grown from the spine at d >= 0.75)
and on config 3 (512^3 value noise; the segment is d >= 0.5), over warm repetitions:

  volume     the HIP-event time of the histogram pass and of the moments' reduction (vx_histogram_stats) and the wall time of the
             whole call for the whole volume with 256 and 4096 bins; the bytes of the resident layout read once (brickf32: 4 B per
             voxel) over the time of the pass, beside the 8 TB/s HBM peak: the fraction of the read floor; beside the wall time of
             the host route, densities rebuilt on the host from the u16 stack + np.histogram
  segment    the same for the segment as the region (the mask's 1 bit per voxel counts as read too), beside segment_mask() +
             host densities + np.histogram
  percentile the wall time of density_percentile(50) of the volume and of the segment (three key passes, moments off) and the
             summed HIP-event time of its passes, beside host densities (+ segment_mask()) + np.percentile(method="lower"), with
             the two results compared bit for bit

One JSON line.  Run from the repository root: python tools/histogram_probe.py [--reps 7] [--skip-256] [--skip-512]"""
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


def host_densities(vox, p):
    """what a host without the device has to rebuild before it can bin anything: the normalised codes of the u16 stack and the
    two fp32 products of d = (volume_density_scale * v) * volume_inv_maj"""
    v = vox.astype(np.float32) * np.float32(1.0 / float(vox.max()))
    return (np.float32(p.volume_density_scale) * v) * np.float32(p.volume_inv_maj)


def host_ms(f, n=3):
    """the wall times of n runs of a host route (slow and steady: three samples)"""
    return [wall_ms(f)[0] for _ in range(n)]


def passes_ms(r, f):
    """f() with the HIP-event times of every vx_histogram pass it makes summed"""
    total = [0.0, 0]
    inner = r._histogram_call

    def counted(q, n):
        out = inner(q, n)
        st = r.histogram_stats()
        total[0] += st[1] + st[2]
        total[1] += 1
        return out
    r._histogram_call = counted
    try:
        ms, out = wall_ms(f)
    finally:
        del r._histogram_call
    return ms, total[0], total[1], out


def run(r, vox, reps):
    p = r.bind_uniforms()
    n = int(vox.size)
    seg = r.segment_mask()
    out = {"voxels": n, "segment_voxels": int(seg.sum())}
    for source, label in (("volume", "volume"), ("segment", "segment")):
        for bins in (256, 4096):
            hist, mom, call = [], [], []
            for i in range(reps + 1):
                ms, h = wall_ms(lambda: r.histogram(bins=bins, source=source))
                st = r.histogram_stats()
                if i:
                    hist.append(st[1]), mom.append(st[2]), call.append(ms)

            def host():
                d = host_densities(vox, p)
                if source == "segment":
                    d = d[r.segment_mask()]
                c, _ = np.histogram(d, bins=bins, range=(0.0, 1.0))
                return c, float(d.mean()), float(d.std())
            route = host_ms(host)
            read = 4 * n + (n // 8 if source == "segment" else 0)
            k = statistics.median(hist)
            out[f"{label}_{bins}"] = {"histogram_ms": spread(hist), "moments_ms": spread(mom), "call_ms": spread(call), "count": h.count,
                                      "bytes_read_once": read, "pass_gbs": round(read / (k * 1e-3) / 1e9, 1),
                                      "read_floor_fraction": round(read / HBM_PEAK / (k * 1e-3), 4), "host_route_ms": spread(route)}
        call, kern = [], []
        for i in range(reps + 1):
            ms, kms, npass, v = passes_ms(r, lambda: r.density_percentile(50.0, source=source))
            if i:
                call.append(ms), kern.append(kms)

        def host_median():
            d = host_densities(vox, p)
            if source == "segment":
                d = d[r.segment_mask()]
            return float(np.percentile(d, 50.0, method="lower"))
        route = host_ms(host_median)
        # the exactness check against the device's own densities is the GPU tests' job; here: the passes and the times
        out[f"{label}_percentile"] = {"call_ms": spread(call), "passes": npass, "passes_kernel_ms": spread(kern), "median_density": v,
                                      "host_route_ms": spread(route)}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-256", action="store_true")
    ap.add_argument("--skip-512", action="store_true")
    a = ap.parse_args()
    from volxel_amd import BENCHMARK_SETTINGS, Volxel3DRenderer, read_u16_stack_to_grid, synth
    out = {}
    for key, n in (("config2_256", 256), ("config3_512", 512)):
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
        out[key] = run(r, vox, a.reps)
        r.close()
        print(f"{key} done", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
