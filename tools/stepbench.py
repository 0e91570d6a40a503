#!/usr/bin/env python3
"""The body-step kernel (ocean_body_step_device, csrc/body.hip k_body_step) against the dynamics kernel it shares its
probe loop with, at cfg3's textures: one velocity context of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/stepbench.py [--launches 20] [--rounds 3] [--markdown] [--parent-lib PATH]

M = 4096 bodies with random poses and motions (tools/bodybench.py's) share OceanContext.box_hull hulls of P = 1, 8
and 64 probes; K = 4, quadratic drag.  Per hull, alternating rounds of
    D   one ocean_body_dynamics_device                       (what a host launches per substep today)
    S1  one ocean_body_step_device with 1 substep            (the integrator's own cost: S1 - D)
    D8  eight ocean_body_dynamics_device back to back        (eight substeps' launches, without the host's round trips)
    S8  one ocean_body_step_device with 8 substeps           (from the same state every time: the bodies do not drift)
Time is the kernels' own (ocean_set_kernel_timing / ocean_kernel_stats kind 2), a round's figure the sum over the
launches of one D, S1, D8 or S8, averaged over `launches` repeats; the reported figure is the median over the rounds,
the spread max - min over the rounds.
Then the largest staged request, 8192 bodies of 64 probes with 8 substeps, through ocean_body_step_async, wall clock
from the call to the landed copy; against it eight ocean_body_dynamics_async round trips one after the other (each
waited for, as a host that integrates on the CPU between them has to), the host's integration and its packing of the
next poses not counted.  With --parent-lib the eight dynamics round trips are also measured in a child process on
that library (a build of the parent commit, in its own tree: ocean-simulation_amd/ocean_hip/liboceanhip.so, whose
Python package the child imports), in the same call.
Prints one JSON line; --markdown appends the tables of docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# (the child of --parent-lib imports the parent's own Python package: this one needs the new symbols to load)
PACKAGE = sys.argv[sys.argv.index("--package") + 1] if "--package" in sys.argv[:-1] else os.path.join(ROOT, "ocean-simulation_amd")
sys.path.insert(0, PACKAGE)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from bodybench import BODIES, CASCADES, HULLS, K, N, random_bodies, summarize  # noqa: E402

SUBSTEPS = 8
vp = ctypes.c_void_p
f32 = np.float32


def random_motion(rng, m):
    return np.concatenate([rng.uniform(-2.0, 2.0, (m, 3)), rng.uniform(-1.0, 1.0, (m, 3))], axis=1).astype(f32)


def step_floats():
    return oh.step_params(1.0 / 480.0, drag=0.5, drag_torque=0.25, linear_damping=0.5, angular_damping=0.25)


def run(ctx, fn, calls, repeats):
    """Mean kernel time in us of one fn(), which makes `calls` launches, over `repeats` back-to-back repeats."""
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(repeats):
        fn()
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == repeats * calls, (cnt, repeats, calls)
    return 1e3 * ms / repeats, ctx.kernel_name(2)


def kernel_table(ctx, launches, rounds):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    bodies, motion = random_bodies(rng, BODIES), random_motion(rng, BODIES)
    state = oh.OceanContext.body_state(bodies, motion)
    props = rng.uniform(0.05, 1.0, (BODIES, 4)).astype(f32)
    sp = step_floats()
    d_bodies, d_motion, d_props = (torch.from_numpy(a).to(dev) for a in (bodies, motion, props))
    d_state0 = torch.from_numpy(state).to(dev)
    out_d = torch.empty(BODIES * 16, dtype=torch.float32, device=dev)
    out_s = torch.empty(BODIES * 32, dtype=torch.float32, device=dev)
    table = []
    for p, (nx, nz) in HULLS:
        hull = oh.OceanContext.box_hull(nx, nz)
        d_hull = torch.from_numpy(hull).to(dev)
        torch.cuda.synchronize()

        def dynamics():
            oh._check(ctx.lib.ocean_body_dynamics_device(ctx._h, 0, oh.QUERY_SURFACE, K, oh.DRAG_QUADRATIC, vp(d_hull.data_ptr()),
                                                         p, vp(d_bodies.data_ptr()), vp(d_motion.data_ptr()), BODIES,
                                                         vp(out_d.data_ptr())), "ocean_body_dynamics_device")

        def step(substeps, src, dst):
            oh._check(ctx.lib.ocean_body_step_device(ctx._h, 0, oh.QUERY_SURFACE, K, oh.DRAG_QUADRATIC, substeps,
                                                     sp.ctypes.data, vp(d_hull.data_ptr()), p, vp(d_props.data_ptr()),
                                                     vp(src.data_ptr()), BODIES, vp(dst.data_ptr())), "ocean_body_step_device")

        def eight_dynamics():
            for _ in range(SUBSTEPS):
                dynamics()

        variants = (("D", dynamics, 1), ("S1", lambda: step(1, d_state0, out_s), 1), ("D8", eight_dynamics, SUBSTEPS),
                    ("S8", lambda: step(SUBSTEPS, d_state0, out_s), 1))
        for _, fn, calls in variants:  # warm-up
            run(ctx, fn, calls, launches)
        torch.cuda.synchronize()
        step(1, d_state0, out_s)
        dynamics()
        torch.cuda.synchronize()
        assert torch.equal(out_s.view(BODIES, 32)[:, 16:], out_d.view(BODIES, 16)), p  # the same record
        times, symbols = {label: [] for label, _, _ in variants}, {}
        for _ in range(rounds):  # alternating rounds
            for label, fn, calls in variants:
                us, symbols[label] = run(ctx, fn, calls, launches)
                times[label].append(us)
        rec = {"probes": p, "bodies": BODIES, "samples": BODIES * p, "substeps": SUBSTEPS, "repeats_per_round": launches}
        for label in times:
            rec[label] = summarize(times[label])
            rec[label]["symbol"] = symbols[label]
        rec["S1"]["ratio_S1_over_D"] = round(rec["S1"]["median_us"] / rec["D"]["median_us"], 3)
        rec["S1"]["no_slower_than_D"] = rec["S1"]["median_us"] <= rec["D"]["median_us"] + rec["D"]["spread_us"]
        rec["S8"]["ratio_D8_over_S8"] = round(rec["D8"]["median_us"] / rec["S8"]["median_us"], 3)
        table.append(rec)
    return table


def dynamics_round_trips(ctx, repeats=20):
    """Eight ocean_body_dynamics_async round trips of 8192 bodies of 64 probes, one after the other."""
    rng = np.random.default_rng(7)
    hull, bodies = oh.OceanContext.box_hull(8, 8), random_bodies(rng, oh.BODY_MAX_BODIES)
    motion = random_motion(rng, oh.BODY_MAX_BODIES)
    slot = oh.PinnedBuffer(len(bodies) * 64)
    wall = []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(SUBSTEPS):
            rb = ctx.body_dynamics_async(hull, bodies, motion, iterations=K, law=oh.DRAG_QUADRATIC, buf=slot)
            rb.wait()
            rb.release()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
    slot.release()
    return {"calls": SUBSTEPS, "bytes_up_per_call": bodies.nbytes + motion.nbytes + hull.nbytes,
            "bytes_down_per_call": len(bodies) * 64, "round_trips_us_median": round(statistics.median(wall), 1),
            "round_trips_us_min": round(min(wall), 1), "requests": repeats}


def async_round_trip(ctx, repeats=20):
    """8192 bodies of 64 probes, 8 substeps, through ocean_body_step_async: 1 MiB of state, 128 KiB of props and 1.25
    KiB of hull up, 1 MiB down; wall clock from the call to the landed copy, and the copy's own time."""
    rng = np.random.default_rng(7)
    hull, bodies = oh.OceanContext.box_hull(8, 8), random_bodies(rng, oh.BODY_MAX_BODIES)
    state = oh.OceanContext.body_state(bodies, random_motion(rng, oh.BODY_MAX_BODIES))
    props = rng.uniform(0.05, 1.0, (len(bodies), 4)).astype(f32)
    sp = step_floats()
    ctx.set_readback_timing(True)
    slot = oh.PinnedBuffer(len(bodies) * 128)
    wall, copy = [], []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.body_step_async(hull, state, props, sp, SUBSTEPS, iterations=K, law=oh.DRAG_QUADRATIC, buf=slot)
        rb.wait()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
            copy.append(1e3 * rb.copy_ms())
        rb.release()
    slot.release()
    ctx.set_readback_timing(False)
    return {"bodies": len(bodies), "probes": len(hull), "substeps": SUBSTEPS,
            "bytes_up": state.nbytes + props.nbytes + hull.nbytes, "bytes_down": len(bodies) * 128,
            "round_trip_us_median": round(statistics.median(wall), 1), "round_trip_us_min": round(min(wall), 1),
            "copy_us_median": round(statistics.median(copy), 1), "requests": repeats}


def markdown(res):
    lines = ["| P | D dynamics (us) | S1 step, 1 substep (us) | S1 / D | D8 eight dynamics (us) | S8 step, 8 substeps (us) | D8 / S8 |",
             "|---|---|---|---|---|---|---|"]
    for rec in res["kernel"]:
        d, s1, d8, s8 = rec["D"], rec["S1"], rec["D8"], rec["S8"]
        lines.append(f"| {rec['probes']} | {d['median_us']:.1f} ± {d['spread_us']:.1f} | {s1['median_us']:.1f} ± {s1['spread_us']:.1f} | "
                     f"{s1['ratio_S1_over_D']} | {d8['median_us']:.1f} ± {d8['spread_us']:.1f} | "
                     f"{s8['median_us']:.1f} ± {s8['spread_us']:.1f} | {s8['ratio_D8_over_S8']} |")
    r, d = res["async_8192x64"], res["dynamics_async_x8"]
    lines += ["", "| 8192 x 64, 8 substeps | bytes up / down | call to landed copy, median / min (us) | copy median (us) |",
              "|---|---|---|---|",
              f"| ocean_body_step_async, 1 request | {r['bytes_up']} / {r['bytes_down']} | {r['round_trip_us_median']} / "
              f"{r['round_trip_us_min']} | {r['copy_us_median']} |",
              f"| ocean_body_dynamics_async, 8 requests | 8 x {d['bytes_up_per_call']} / 8 x {d['bytes_down_per_call']} | "
              f"{d['round_trips_us_median']} / {d['round_trips_us_min']} | |"]
    if "dynamics_async_x8_parent" in res:
        d = res["dynamics_async_x8_parent"]
        lines.append(f"| the same on the parent's library | 8 x {d['bytes_up_per_call']} / 8 x {d['bytes_down_per_call']} | "
                     f"{d['round_trips_us_median']} / {d['round_trips_us_min']} | |")
    return "\n".join(lines)


def water(velocity=True):
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, readback="height", velocity=velocity).Awake()
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    return wb


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="repeats per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    ap.add_argument("--parent-lib", help="a liboceanhip.so of the parent commit: its eight dynamics round trips, in a child process")
    ap.add_argument("--dynamics-only", action="store_true", help=argparse.SUPPRESS)  # the child of --parent-lib
    ap.add_argument("--package", help=argparse.SUPPRESS)  # ... and the directory of the ocean_hip package it imports
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("stepbench.py needs a GPU: it measures")
    wb = water()
    try:
        if args.dynamics_only:
            print(json.dumps(dynamics_round_trips(wb.ctx)))
            return
        launches, rounds = max(20, args.launches), max(3, args.rounds)
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures), {BODIES} bodies, K = {K}, quadratic drag",
               "device": torch.cuda.get_device_name(0), "kernel": kernel_table(wb.ctx, launches, rounds),
               "async_8192x64": async_round_trip(wb.ctx), "dynamics_async_x8": dynamics_round_trips(wb.ctx)}
    finally:
        wb.OnDisable()
    if args.parent_lib:
        lib = os.path.abspath(args.parent_lib)
        child = subprocess.run([sys.executable, os.path.abspath(__file__), "--dynamics-only", "--package",
                                os.path.dirname(os.path.dirname(lib))], capture_output=True, text=True,
                               env=dict(os.environ, OCEAN_HIP_LIB=lib), timeout=600)
        if child.returncode != 0:
            sys.exit("stepbench.py: the parent library's run failed:\n" + child.stderr)
        res["dynamics_async_x8_parent"] = json.loads(child.stdout.strip().splitlines()[-1])
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
