#!/usr/bin/env python3
"""The WaterBody Update loop at cfg3 with readback "probes" (one ocean_query_surface_async per frame in
place of the slice readback), beside the loop bench.py times with readback "height".

    python tools/probe_loop.py [--steps 500] [--warmup 50] [--parent-height FPS]

--steps / --warmup mean what they mean to bench.py: the loops time max(50, steps // 2) Update frames after a
warm-up of at least `warmup` frames and bench.UPDATE_WARM_S seconds, every request landed inside the timed
region.  Prints one JSON line: frames/s of the probes loop for M = 16, 1024 and 65536 probes (surface mode,
4 steps), the height loop of this tree run the same way, the query kernels' own time (the device form timed
by ocean_kernel_stats kind 2 on a context without mip chains, so kind 2 holds nothing else), and
--parent-height: `update_loop.height.frames_per_s` of `python bench.py --full` on the parent commit, taken
on the same box in the same session, recorded as given.  A record, not a gate (docs/MEASUREMENTS.md)."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))
sys.path.insert(0, ROOT)

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from bench import UPDATE_WARM_S  # noqa: E402

M_VALUES = (16, 1024, 65536)


def bodies(m, seed=1):
    rng = np.random.default_rng(seed)
    p = np.zeros((m, 3), np.float32)
    p[:, 0] = rng.uniform(-2000.0, 2000.0, m)
    p[:, 2] = rng.uniform(-2000.0, 2000.0, m)
    return p


def timed_loop(wb, steps, warmup):
    f = 0
    w0 = time.perf_counter()
    while f < max(warmup, 2 * len(wb._ring)) or time.perf_counter() - w0 < UPDATE_WARM_S:
        wb.Update(f / 60.0)
        f += 1
    wb.WaitForReadback()
    t0 = time.perf_counter()
    for k in range(steps):
        wb.Update((f + k) / 60.0)
    wb.WaitForReadback()
    s = (time.perf_counter() - t0) / steps
    return {"frames_per_s": round(1.0 / s, 2), "ms_per_frame": round(1e3 * s, 4), "timed_frames": steps,
            "warmup_frames": f}


def kernel_times(launches=200):
    """The query kernels alone at cfg3's textures: device-form launches back to back, HIP events per launch."""
    wb = oh.scene_water_body(n=1024, n_cascades=4, seed=20251121, mips=False, readback="probes").Awake()
    ctx = wb.ctx
    ctx.step(0.5)
    dev = torch.device("cuda", ctx.device)
    out = {}
    vp = ctypes.c_void_p
    for m in M_VALUES:
        p = torch.from_numpy(np.ascontiguousarray(bodies(m)[:, [0, 2]])).to(dev)
        o = torch.empty(m * 8, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        rec = {}
        for name, mode, iters in (("surface_k4", oh.QUERY_SURFACE, 4), ("surface_k0", oh.QUERY_SURFACE, 0),
                                  ("surface_k16", oh.QUERY_SURFACE, 16), ("reference", oh.QUERY_REFERENCE, 0)):
            for _ in range(20):
                oh._check(ctx.lib.ocean_query_surface_device(ctx._h, 0, mode, iters, vp(p.data_ptr()), m,
                                                             vp(o.data_ptr())), "ocean_query_surface_device")
            ctx.synchronize()
            ctx.set_kernel_timing(True)
            ctx.kernel_stats(2)
            for _ in range(launches):
                oh._check(ctx.lib.ocean_query_surface_device(ctx._h, 0, mode, iters, vp(p.data_ptr()), m,
                                                             vp(o.data_ptr())), "ocean_query_surface_device")
            ms, cnt = ctx.kernel_stats(2)
            ctx.set_kernel_timing(False)
            rec[name] = {"us": round(1e3 * ms / cnt, 2), "launches": cnt, "symbol": ctx.kernel_name(2)}
        out[str(m)] = rec
    wb.OnDisable()
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=500)
    ap.add_argument("--warmup", type=int, default=50)
    ap.add_argument("--parent-height", type=float, default=None,
                    help="update_loop.height.frames_per_s of bench.py --full on the parent commit (same box, same session)")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("probe_loop.py needs a GPU: it measures")
    steps = max(50, args.steps // 2)
    out = {"workload": "cfg3 (4 x 1024^2) frame + GenerateMips + one request per frame, ocean_hip.WaterBody.Update",
           "probes": {}, "parent_height_frames_per_s": args.parent_height}
    for m in M_VALUES:
        wb = oh.scene_water_body(n=1024, n_cascades=4, seed=20251121, readback="probes", probeCapacity=m)
        wb.SetProbes(bodies(m))
        wb.Awake()
        try:
            rec = timed_loop(wb, steps, args.warmup)
            rec["pcie_bytes_per_frame"] = {"up": m * 8, "down": m * 32}
            rec["max_residual_m"] = float(wb.ProbeResults[:, 3].max())
            out["probes"][str(m)] = rec
        finally:
            wb.OnDisable()
    wb = oh.scene_water_body(n=1024, n_cascades=4, seed=20251121, readback="height").Awake()
    try:
        out["height"] = timed_loop(wb, steps, args.warmup)
        out["height"]["pcie_bytes_per_frame"] = {"up": 0, "down": 1024 * 1024 * 4}
    finally:
        wb.OnDisable()
    out["query_kernel"] = kernel_times()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
