#!/usr/bin/env python3
"""The surface velocity (OCEAN_F_VELOCITY, csrc/velocity.hip) at cfg3's shape and parameters: one context of
4 x 1024^2 with the scene's cascades, full outputs.

    python tools/velbench.py [--steps 200] [--rounds 3] [--launches 20] [--no-trace] [--markdown]

1. ocean_step frames/s without and with OCEAN_F_VELOCITY (and with OCEAN_VEL_NT=1, the pack kernel's streamed
   stores): after a pre-warm, `rounds` alternating rounds of `steps` steps each, wall clock around the
   synchronized loop; the figure is the median over the rounds, the spread max - min.
2. The velocity launches' own times.  By events (ocean_set_kernel_timing): kind 2 of a velocity step is the four
   launches together, evolve + rows + columns + pack; the operator's share is read from ocean_ifft2d over PLANE0
   and PLANE1 of the same context, the identical two launches over the same 2 U unit-planes (kinds 0 and 1).  Per
   kernel (unless --no-trace): a child run of this script under `rocprofv3 --kernel-trace --stats` that steps a
   velocity context only; its k_rows2 / k_cols2 records are the velocity's operator launches (the fused frame
   runs other kernels).
3. ocean_query_velocity_device against ocean_query_surface_device over the same 65,536 points at K = 4, kernel
   time by events, alternating rounds as tools/bodybench.py.
Prints one JSON line; --markdown appends the tables of docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import csv
import ctypes
import glob
import json
import os
import shutil
import statistics
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402

N, CASCADES, POINTS, K = 1024, 4, 65536, 4
PREWARM_S = 1.0
vp = ctypes.c_void_p
f32 = np.float32


def make_context(flags):
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES)
    ctx = oh.OceanContext(N, CASCADES, 1, flags)
    ctx.set_params(wb.params(), [c.as_dict() for c in wb.cascades])
    ctx.generate_noise(20251121)
    ctx.init_spectrum()
    ctx.synchronize()
    return ctx


def summarize(rounds, digits=2):
    return {"median": round(statistics.median(rounds), digits), "spread": round(max(rounds) - min(rounds), digits),
            "rounds": [round(r, digits) for r in rounds]}


def prewarm(ctxs):
    p0, f = time.perf_counter(), 0
    while time.perf_counter() - p0 < PREWARM_S:
        for ctx in ctxs:
            for _ in range(8):
                ctx.step(-1.0 - f / 60.0)
                f += 1
            ctx.synchronize()
    for ctx in ctxs:
        ctx.reset_foam()


def frames_per_second(variants, steps, rounds):
    """variants: [(label, ctx)] -> {label: frames/s summary}; alternating rounds."""
    prewarm([c for _, c in variants])
    fps = {label: [] for label, _ in variants}
    for r in range(rounds):
        for label, ctx in variants:
            for f in range(10):
                ctx.step(f / 60.0)
            ctx.synchronize()
            t0 = time.perf_counter()
            for f in range(steps):
                ctx.step((10 + f) / 60.0)
            ctx.synchronize()
            fps[label].append(steps / (time.perf_counter() - t0))
    return {label: summarize(v, 1) for label, v in fps.items()}


def event_times(ctx, steps):
    """us per step by kind over `steps` steps, then the operator's two launches over PLANE0 and PLANE1."""
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    for k in range(3):
        ctx.kernel_stats(k)
    for f in range(steps):
        ctx.step(f / 60.0)
    step = [ctx.kernel_stats(k) for k in range(3)]
    for _ in range(steps):
        ctx.ifft2d(0b11)
    op = [ctx.kernel_stats(k) for k in range(2)]
    ctx.set_kernel_timing(False)
    return {"steps": steps,
            "pass_a_us": round(1e3 * step[0][0] / steps, 2), "pass_b_us": round(1e3 * step[1][0] / steps, 2),
            "velocity_kind2_us": round(1e3 * step[2][0] / steps, 2), "velocity_launches_per_step": step[2][1] / steps,
            "operator_rows_us": round(1e3 * op[0][0] / steps, 2), "operator_cols_us": round(1e3 * op[1][0] / steps, 2),
            "evolve_plus_pack_us": round(1e3 * (step[2][0] - op[0][0] - op[1][0]) / steps, 2)}


def trace_child(steps):
    ctx = make_context(oh.F_VELOCITY)
    for f in range(steps):
        ctx.step(f / 60.0)
    ctx.synchronize()
    ctx.close()


def trace(steps):
    """Per-kernel average us of a velocity context's steps from a child run under rocprofv3, or the reason
    there is none."""
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"skipped": "rocprofv3 not found"}
    out = tempfile.mkdtemp(prefix="velbench_trace_")
    try:
        r = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "run", "--",
                            sys.executable, os.path.abspath(__file__), "--trace-child", "--steps", str(steps)],
                           capture_output=True, text=True, timeout=280)
        files = glob.glob(os.path.join(out, "**", "run_kernel_stats.csv"), recursive=True)
        if r.returncode != 0 or not files:
            return {"skipped": f"rocprofv3 exit {r.returncode}", "stderr": r.stderr[-300:]}
        res = {}
        for row in csv.DictReader(open(files[0])):
            for key in ("k_evolve_velocity", "k_rows2", "k_cols2", "k_pack_velocity", "k_pass_a", "k_pass_b"):
                if key in row["Name"]:
                    res[key] = {"calls": int(row["Calls"]), "avg_us": round(float(row["AverageNs"]) / 1e3, 2)}
        return res
    finally:
        shutil.rmtree(out, ignore_errors=True)


def run_kernel(ctx, fn, launches):
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(launches):
        oh._check(fn(), "launch")
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == launches, (cnt, launches)
    return 1e3 * ms / cnt


def query_table(ctx, launches, rounds):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    q = rng.uniform(-2000.0, 2000.0, (POINTS, 2)).astype(f32)
    d_q = torch.from_numpy(q).to(dev)
    out_a = torch.empty(POINTS * 8, dtype=torch.float32, device=dev)
    out_b = torch.empty(POINTS * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    variants = (
        ("surface", lambda: ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), POINTS,
                                                               vp(out_a.data_ptr()))),
        ("velocity", lambda: ctx.lib.ocean_query_velocity_device(ctx._h, 0, K, vp(d_q.data_ptr()), POINTS,
                                                                 vp(out_b.data_ptr()))),
    )
    for _, fn in variants:
        run_kernel(ctx, fn, launches)
    torch.cuda.synchronize()
    a, b = out_a.view(POINTS, 8), out_b.view(POINTS, 8)
    assert torch.equal(a[:, [3, 0, 1, 2]], b[:, 3:7])  # the same fixed point: residual, height, p
    times = {label: [] for label, _ in variants}
    for _ in range(rounds):
        for label, fn in variants:
            times[label].append(run_kernel(ctx, fn, launches))
    res = {label: summarize(v) for label, v in times.items()}
    res["points"], res["launches_per_round"] = POINTS, launches
    res["velocity_over_surface"] = round(res["velocity"]["median"] / res["surface"]["median"], 3)
    return res


def markdown(res):
    f, e, q = res["frames_per_s"], res["events"], res["query"]
    lines = ["| ocean_step | frames/s (median ± spread) | ms per frame |", "|---|---|---|"]
    for label in f:
        lines.append(f"| {label} | {f[label]['median']:.0f} ± {f[label]['spread']:.0f} | {1e3 / f[label]['median']:.4f} |")
    lines += ["", "| by events, per step (us) | |", "|---|---|",
              f"| pass A / pass B (kinds 0 / 1) | {e['pass_a_us']} / {e['pass_b_us']} |",
              f"| the four velocity launches (kind 2) | {e['velocity_kind2_us']} |",
              f"| operator rows / columns over 2 U unit-planes (ocean_ifft2d) | {e['operator_rows_us']} / {e['operator_cols_us']} |",
              f"| evolve + pack (the remainder) | {e['evolve_plus_pack_us']} |"]
    t = res.get("trace", {})
    if "k_evolve_velocity" in t:
        lines += ["", "| rocprofv3, velocity context | calls | average (us) |", "|---|---|---|"]
        lines += [f"| {k} | {v['calls']} | {v['avg_us']} |" for k, v in t.items()]
    lines += ["", f"| {q['points']} points, K = {K} | kernel (us, median ± spread) |", "|---|---|",
              f"| ocean_query_surface_device | {q['surface']['median']} ± {q['surface']['spread']} |",
              f"| ocean_query_velocity_device | {q['velocity']['median']} ± {q['velocity']['spread']} |"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=20, help="query launches per round (at least 20)")
    ap.add_argument("--no-trace", action="store_true")
    ap.add_argument("--trace-child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("velbench.py needs a GPU: it measures")
    if args.trace_child:
        return trace_child(args.steps)
    steps, rounds, launches = max(20, args.steps), max(3, args.rounds), max(20, args.launches)
    plain, vel = make_context(0), make_context(oh.F_VELOCITY)
    os.environ["OCEAN_VEL_NT"] = "1"  # read once, in ocean_create
    vel_nt = make_context(oh.F_VELOCITY)
    del os.environ["OCEAN_VEL_NT"]
    try:
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 shape and parameters), full outputs",
               "device": torch.cuda.get_device_name(0), "steps_per_round": steps, "rounds": rounds,
               "frames_per_s": frames_per_second([("plain", plain), ("OCEAN_F_VELOCITY", vel),
                                                  ("OCEAN_F_VELOCITY, OCEAN_VEL_NT=1", vel_nt)], steps, rounds),
               "events": event_times(vel, steps), "events_vel_nt": event_times(vel_nt, steps),
               "query": query_table(vel, launches, rounds)}
        p, v = res["frames_per_s"]["plain"]["median"], res["frames_per_s"]["OCEAN_F_VELOCITY"]["median"]
        res["step_time_ratio"] = round(p / v, 3)
    finally:
        for c in (plain, vel, vel_nt):
            c.close()
    if not args.no_trace:
        res["trace"] = trace(50)
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
