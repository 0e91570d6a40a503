#!/usr/bin/env python3
"""Dense control for the band-limited-cascade pruning (docs/MEASUREMENTS.md section 13): cfg3's shape
(4 x 1024^2) with the scene's wavelengths but every cascade's band opened to 1e-10 .. 1e12, so that no row
of any spectrum is all zero and the frame must run today's dense kernels.  Timed as bench.py times its
headline: pre-warm, warm-up, then --steps frames between two synchronizes.  One JSON line.
    OCEAN_HIP_LIB=<library> python tools/prunebench.py [--steps 500] [--warmup 50]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (torch first, then ocean_hip: one HIP runtime per process)
from bench import oh  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    args = ap.parse_args()
    cas = [dict(c, cutoff_low=1e-10, cutoff_high=1e12) for c in bench.SCENE_CASCADES]
    ctx = oh.OceanContext(1024, len(cas), 1, 0, device=0)
    ctx.set_params(bench.SCENE_PARAMS, cas)
    ctx.generate_noise(bench.tile_seed(20251121, 0))
    ctx.init_spectrum()
    ctx.synchronize()
    frames, p0 = 0, time.perf_counter()
    while time.perf_counter() - p0 < bench.PREWARM_S:
        for _ in range(8):
            ctx.step(-1.0 - frames / 60.0)
            frames += 1
        ctx.synchronize()
    ctx.reset_foam()
    for f in range(args.warmup):
        ctx.step(f / 60.0)
    ctx.synchronize()
    t0 = time.perf_counter()
    for f in range(args.steps):
        ctx.step((args.warmup + f) / 60.0)
    ctx.synchronize()
    elapsed = time.perf_counter() - t0
    # the same frames again with kernel events (outside the timed region, as bench.py --full)
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(0), ctx.kernel_stats(1)
    for f in range(args.steps):
        ctx.step((args.warmup + args.steps + f) / 60.0)
    ctx.synchronize()
    a_ms, b_ms = ctx.kernel_stats(0)[0], ctx.kernel_stats(1)[0]
    ctx.set_kernel_timing(False)
    print(json.dumps({"workload": "dense control: 4 x 1024^2, bands 1e-10 .. 1e12", "steps": args.steps,
                      "value": round(args.steps / elapsed, 2), "unit": "frames/s",
                      "ms_per_step": round(1e3 * elapsed / args.steps, 5),
                      "kernels_us": {"pass_a": round(1e3 * a_ms / args.steps, 3),
                                     "pass_b": round(1e3 * b_ms / args.steps, 3)},
                      "kernels": [ctx.kernel_name(0), ctx.kernel_name(1)],
                      "library": os.environ.get("OCEAN_HIP_LIB", "default")}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
