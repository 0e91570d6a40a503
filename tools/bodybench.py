#!/usr/bin/env python3
"""The body kernel (ocean_body_buoyancy_device, csrc/body.hip) against the point query over the same probe
positions, at cfg3's textures: one context of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/bodybench.py [--launches 20] [--rounds 3] [--markdown]

M = 4096 bodies with random poses (unit quaternions, scales in [0.5, 3], origins within +-2000 m, cy within
+-1 m) share OceanContext.box_hull hulls of P = 1, 8 and 64 probes; K = 4.  B is the body kernel.  A is
ocean_query_surface_device over the same M x P world positions, formed on the host in fp32 with ocean.h's
formulas and uploaded once: the same taps, 8 B read and 32 B written per probe instead of 40 B read and 32 B
written per body -- and the host still has the transform before it and the reduction after it to do.

Time is the kernels' own (ocean_set_kernel_timing / ocean_kernel_stats kind 2: events on the dispatch itself).
After a warm-up of both, `rounds` alternating rounds A, B of `launches` back-to-back launches each; a round's
figure is its mean per launch, the reported figure the median over the rounds, the spread max - min over the
rounds.  B is "no slower" when its median does not exceed A's by more than A's spread.  Also: the round trip
of the largest request, 8192 bodies of 64 probes, through ocean_body_buoyancy_async (call to landed data, wall
clock, and the copy's own time from ocean_readback_copy_ms).
The dynamics line (ocean_body_dynamics_device, k_body_dynamics) runs on a second context with OCEAN_F_VELOCITY over
the same bodies and hulls, with random motions: D is the dynamics kernel, and against it stands what a host issues
today for the same numbers, B + V in the same run: the body kernel and ocean_query_velocity_device over the same
M x P probe positions (before the host's own transform and its reduction of M x P x 32 B).
Prints one JSON line; --markdown appends the tables of docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402

N, CASCADES, BODIES, K = 1024, 4, 4096, 4
HULLS = ((1, (1, 1)), (8, (4, 2)), (64, (8, 8)))  # P: box_hull(nx, nz)
vp = ctypes.c_void_p
f32 = np.float32


def random_bodies(rng, m):
    b = np.empty((m, 10), f32)
    b[:, 0] = rng.uniform(-2000.0, 2000.0, m)
    b[:, 1] = rng.uniform(-1.0, 1.0, m)
    b[:, 2] = rng.uniform(-2000.0, 2000.0, m)
    q = rng.standard_normal((m, 4))
    b[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    b[:, 7:10] = rng.uniform(0.5, 3.0, (m, 3))
    return b


def probe_positions(hull, bodies):
    """(w.x, w.z) of every probe of every body, float32[M * P][2], with ocean.h's fp32 formulas."""
    h, b = hull[None, :, :], bodies[:, None, :]
    two = f32(2.0)

    def cross(u, a):
        return (u[1] * a[2] - u[2] * a[1], u[2] * a[0] - u[0] * a[2], u[0] * a[1] - u[1] * a[0])
    u, qw = (b[..., 3], b[..., 4], b[..., 5]), b[..., 6]
    a = (b[..., 7] * h[..., 0], b[..., 8] * h[..., 1], b[..., 9] * h[..., 2])
    t = tuple(two * c for c in cross(u, a))
    ut = cross(u, t)
    d = tuple((a[i] + qw * t[i]) + ut[i] for i in range(3))
    return np.ascontiguousarray(np.stack([(b[..., 0] + d[0]).ravel(), (b[..., 2] + d[2]).ravel()], axis=1), f32)


def run(ctx, fn, launches):
    """Mean kernel time per launch in us over `launches` back-to-back launches, and the kernel's symbol."""
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(launches):
        oh._check(fn(), "launch")
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == launches, (cnt, launches)
    return 1e3 * ms / cnt, ctx.kernel_name(2)


def summarize(rounds):
    return {"median_us": round(statistics.median(rounds), 2), "spread_us": round(max(rounds) - min(rounds), 2),
            "rounds_us": [round(r, 2) for r in rounds]}


def kernel_table(ctx, launches, rounds):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    bodies = random_bodies(rng, BODIES)
    d_bodies = torch.from_numpy(bodies).to(dev)
    out_b = torch.empty(BODIES * 8, dtype=torch.float32, device=dev)
    table = []
    for p, (nx, nz) in HULLS:
        hull = oh.OceanContext.box_hull(nx, nz)
        q = probe_positions(hull, bodies)
        m = len(q)
        d_hull, d_q = torch.from_numpy(hull).to(dev), torch.from_numpy(q).to(dev)
        out_a = torch.empty(m * 8, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        variants = (
            ("A", lambda: ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), m,
                                                             vp(out_a.data_ptr()))),
            ("B", lambda: ctx.lib.ocean_body_buoyancy_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_hull.data_ptr()), p,
                                                             vp(d_bodies.data_ptr()), BODIES, vp(out_b.data_ptr()))),
        )
        for _, fn in variants:  # warm-up
            run(ctx, fn, launches)
        # the worst residual of a body is the largest of its probes' in the point query: the same lookups
        torch.cuda.synchronize()
        assert torch.equal(out_a.view(BODIES, p, 8)[:, :, 3].max(dim=1).values, out_b.view(BODIES, 8)[:, 7]), p
        times, symbols = {"A": [], "B": []}, {}
        for _ in range(rounds):  # alternating rounds
            for label, fn in variants:
                us, symbols[label] = run(ctx, fn, launches)
                times[label].append(us)
        rec = {"probes": p, "bodies": BODIES, "samples": m, "launches_per_round": launches}
        for label in times:
            rec[label] = summarize(times[label])
            rec[label]["symbol"] = symbols[label]
        a, b = rec["A"], rec["B"]
        b["no_slower_than_A"] = b["median_us"] <= a["median_us"] + a["spread_us"]
        b["ratio_A_over_B"] = round(a["median_us"] / b["median_us"], 3)
        table.append(rec)
    return table


def dynamics_table(ctx, launches, rounds):
    """D = ocean_body_dynamics_device against B + V = ocean_body_buoyancy_device + ocean_query_velocity_device over
    the same probe positions, on a velocity context: alternating rounds B, V, D."""
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    bodies = random_bodies(rng, BODIES)
    motion = np.concatenate([rng.uniform(-2.0, 2.0, (BODIES, 3)), rng.uniform(-1.0, 1.0, (BODIES, 3))], axis=1).astype(f32)
    d_bodies, d_motion = torch.from_numpy(bodies).to(dev), torch.from_numpy(motion).to(dev)
    out_b = torch.empty(BODIES * 8, dtype=torch.float32, device=dev)
    out_d = torch.empty(BODIES * 16, dtype=torch.float32, device=dev)
    table = []
    for p, (nx, nz) in HULLS:
        hull = oh.OceanContext.box_hull(nx, nz)
        q = probe_positions(hull, bodies)
        m = len(q)
        d_hull, d_q = torch.from_numpy(hull).to(dev), torch.from_numpy(q).to(dev)
        out_v = torch.empty(m * 8, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        variants = (
            ("B", lambda: ctx.lib.ocean_body_buoyancy_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_hull.data_ptr()), p,
                                                             vp(d_bodies.data_ptr()), BODIES, vp(out_b.data_ptr()))),
            ("V", lambda: ctx.lib.ocean_query_velocity_device(ctx._h, 0, K, vp(d_q.data_ptr()), m, vp(out_v.data_ptr()))),
            ("D", lambda: ctx.lib.ocean_body_dynamics_device(ctx._h, 0, oh.QUERY_SURFACE, K, oh.DRAG_QUADRATIC,
                                                             vp(d_hull.data_ptr()), p, vp(d_bodies.data_ptr()),
                                                             vp(d_motion.data_ptr()), BODIES, vp(out_d.data_ptr()))),
        )
        for _, fn in variants:  # warm-up
            run(ctx, fn, launches)
        torch.cuda.synchronize()
        assert torch.equal(out_d.view(BODIES, 16)[:, :8], out_b.view(BODIES, 8)), p  # the same buoyancy record
        times, symbols = {"B": [], "V": [], "D": []}, {}
        for _ in range(rounds):  # alternating rounds
            for label, fn in variants:
                us, symbols[label] = run(ctx, fn, launches)
                times[label].append(us)
        rec = {"probes": p, "bodies": BODIES, "samples": m, "launches_per_round": launches}
        for label in times:
            rec[label] = summarize(times[label])
            rec[label]["symbol"] = symbols[label]
        both = [b + v for b, v in zip(times["B"], times["V"])]
        rec["B_plus_V"] = summarize(both)
        d = rec["D"]
        d["below_B_plus_V"] = d["median_us"] < rec["B_plus_V"]["median_us"]
        d["ratio_BV_over_D"] = round(rec["B_plus_V"]["median_us"] / d["median_us"], 3)
        d["ratio_D_over_B"] = round(d["median_us"] / rec["B"]["median_us"], 3)
        table.append(rec)
    return table


def async_round_trip(ctx, repeats=20):
    """8192 bodies of 64 probes through ocean_body_buoyancy_async: 320 KiB of bodies and 1.25 KiB of hull up,
    256 KiB down; wall clock from the call to the landed copy, and the copy's own time."""
    rng = np.random.default_rng(7)
    hull, bodies = oh.OceanContext.box_hull(8, 8), random_bodies(rng, oh.BODY_MAX_BODIES)
    ctx.set_readback_timing(True)
    slot = oh.PinnedBuffer(len(bodies) * 32)
    wall, copy = [], []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.body_buoyancy_async(hull, bodies, iterations=K, buf=slot)
        rb.wait()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
            copy.append(1e3 * rb.copy_ms())
        rb.release()
    slot.release()
    ctx.set_readback_timing(False)
    return {"bodies": len(bodies), "probes": len(hull), "bytes_up": bodies.nbytes + hull.nbytes, "bytes_down": len(bodies) * 32,
            "round_trip_us_median": round(statistics.median(wall), 1), "round_trip_us_min": round(min(wall), 1),
            "copy_us_median": round(statistics.median(copy), 1), "requests": repeats}


def markdown(res):
    lines = ["| P | samples | A point query (us) | B body kernel (us) | A / B | no slower |", "|---|---|---|---|---|---|"]
    for rec in res["kernel"]:
        a, b = rec["A"], rec["B"]
        lines.append(f"| {rec['probes']} | {rec['samples']} | {a['median_us']:.1f} ± {a['spread_us']:.1f} | "
                     f"{b['median_us']:.1f} ± {b['spread_us']:.1f} | {b['ratio_A_over_B']} | {b['no_slower_than_A']} |")
    if "dynamics" in res:
        lines += ["", "| P | samples | B body kernel (us) | V velocity query (us) | B + V (us) | D dynamics kernel (us) | "
                  "(B + V) / D | D / B | D below B + V |", "|---|---|---|---|---|---|---|---|---|"]
        for rec in res["dynamics"]:
            b, v, s, d = rec["B"], rec["V"], rec["B_plus_V"], rec["D"]
            lines.append(f"| {rec['probes']} | {rec['samples']} | {b['median_us']:.1f} ± {b['spread_us']:.1f} | "
                         f"{v['median_us']:.1f} ± {v['spread_us']:.1f} | {s['median_us']:.1f} ± {s['spread_us']:.1f} | "
                         f"{d['median_us']:.1f} ± {d['spread_us']:.1f} | {d['ratio_BV_over_D']} | {d['ratio_D_over_B']} | "
                         f"{d['below_B_plus_V']} |")
    r = res["async_8192x64"]
    lines += ["", "| 8192 x 64 async | bytes up / down | round trip median / min (us) | copy median (us) |", "|---|---|---|---|",
              f"| K = {K} | {r['bytes_up']} / {r['bytes_down']} | {r['round_trip_us_median']} / {r['round_trip_us_min']} | "
              f"{r['copy_us_median']} |"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="launches per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bodybench.py needs a GPU: it measures")
    launches, rounds = max(20, args.launches), max(3, args.rounds)
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, readback="height").Awake()
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    try:
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures), {BODIES} bodies, K = {K}",
               "device": torch.cuda.get_device_name(0), "kernel": kernel_table(wb.ctx, launches, rounds),
               "async_8192x64": async_round_trip(wb.ctx)}
    finally:
        wb.OnDisable()
    wv = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, readback="height", velocity=True).Awake()
    wv.ctx.step(0.5)
    wv.ctx.step(1.0)
    wv.ctx.synchronize()
    try:
        res["dynamics"] = dynamics_table(wv.ctx, launches, rounds)
    finally:
        wv.OnDisable()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
