#!/usr/bin/env python3
"""The spray particles (ocean_spray_step_device, csrc/spray.hip) against what a host has today for the same frame, at
cfg3's textures: velocity contexts of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/spraybench.py [--launches 20] [--rounds 3] [--markdown]

A is today's yardstick: S launches of ocean_query_surface_device (K = 2) over the particles' positions, which leave
the integration, the compare and the compaction to the host (and the landing of 32 B per particle and substep,
which is not priced here).  B is one ocean_spray_step_device call of S substeps: its three launches (step, scan,
emit), with the air skip on (the default) and off (a context created under OCEAN_RAY_BOUNDS=0).  Pools of 65,535 and
1,048,575 particles, S = 1 and 4, and two clouds: a low one, every particle between the water under it and H (the
height no wave reaches), and a high one, every particle above H.  The particles drift at 1 m/s with g = kd = 0 and a
long life, so that nearly all of them take every substep.

Prediction, written before the first run: below H a substep costs the query's K + 1 dependent gathers, so B at S = 1
should cost about A plus the two 32 B record moves per particle and the scan, 1.0 to 1.3 x A, and the same with the
skip off; above H with the skip on a substep samples nothing, so B should be bound by its 32 B load, 32 B scratch store
and 64 B emit copy per particle and cost a small fraction of A (a tenth or less at a million particles), and barely
grow with S.

Time is the kernels' own (ocean_set_kernel_timing / ocean_kernel_stats kind 2).  After a warm-up of every variant,
`rounds` alternating rounds of `launches` back-to-back calls each; a round's figure is its mean per call, the
reported figure the median over the rounds, the spread max - min over the rounds.  Also the round trip of one pool of
65,535 through ocean_spray_step_async.  Prints one JSON line; --markdown appends the table of docs/MEASUREMENTS.md.
A record, not a gate."""
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

N, CASCADES, K = 1024, 4, 2
POOLS = (oh.SPRAY_MAX_STAGED, oh.SPRAY_MAX_PARTICLES)
SUBSTEPS = (1, 4)
SPRAY = oh.OceanContext.spray_params(1.0 / 240.0, 0.0, 0.0, (0.0, 0.0, 0.0), 1e6, 1.0, 0.0)
vp = ctypes.c_void_p


def run(ctx, fn, launches, per_call=1):
    """Mean kernel time per call in us over `launches` back-to-back calls of `per_call` timed entries each."""
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(launches):
        fn()
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == launches * per_call, (cnt, launches, per_call)
    return 1e3 * ms / launches


def summarize(rounds):
    return {"median_us": round(statistics.median(rounds), 2), "spread_us": round(max(rounds) - min(rounds), 2),
            "rounds_us": [round(r, 2) for r in rounds]}


def make_body(env):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, velocity=True,
                                 readback="height").Awake()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    return wb


def air_height(ctx):
    b = ctx.surface_bounds()
    top, mag = np.float32(0), np.float32(0)
    for c in range(len(b)):
        top = top + b[c, 5]
        mag = mag + max(abs(b[c, 1]), abs(b[c, 5]))
    return np.float32(top + mag * np.float32(2.0 ** -19))


def clouds(ctx, count, dev):
    """{"low": pool, "high": pool} float32[count + 1][8] and the positions float32[count][2], all on the device."""
    rng = np.random.default_rng(count)
    q = rng.uniform(-2000.0, 2000.0, (count, 2)).astype(np.float32)
    d_q = torch.from_numpy(q).to(dev)
    d_rec = torch.empty(count * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    oh._check(ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), count,
                                                 vp(d_rec.data_ptr())), "ocean_query_surface_device")
    ctx.synchronize()
    eta = d_rec.cpu().numpy().reshape(count, 8)[:, 0]
    H = float(air_height(ctx))
    u = rng.uniform(0.0, 1.0, count).astype(np.float32)
    ang = rng.uniform(0.0, 2 * np.pi, count)
    pools = {}
    for name, y in (("low", eta + np.float32(0.02) + u * np.float32(0.9) * np.maximum(np.float32(H) - eta - np.float32(0.02), 0)),
                    ("high", np.float32(H + 0.5) + np.float32(10.0) * u)):
        rec = np.zeros((count, 8), np.float32)
        rec[:, 0], rec[:, 1], rec[:, 2] = q[:, 0], y, q[:, 1]
        rec[:, 4], rec[:, 6] = np.cos(ang), np.sin(ang)
        rec[:, 7] = np.arange(count, dtype=np.float32)
        pools[name] = torch.from_numpy(oh.OceanContext.spray_pool(rec, count)).to(dev)
    torch.cuda.synchronize()
    return pools, d_q, d_rec, H


def measure(bodies, launches, rounds):
    on, off = bodies["on"].ctx, bodies["off"].ctx
    dev = torch.device("cuda", on.device)
    table = []
    for count in POOLS:
        pools, d_q, d_rec, H = clouds(on, count, dev)
        d_out = torch.empty((count + 1) * 8, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        for S in SUBSTEPS:
            def query():
                for _ in range(S):
                    oh._check(on.lib.ocean_query_surface_device(on._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), count,
                                                                vp(d_rec.data_ptr())), "ocean_query_surface_device")
            variants = [("A: S query launches", on, query, S)]
            for cloud, pool in pools.items():
                for label, ctx in (("skip on", on), ("skip off", off)):
                    def fn(ctx=ctx, pool=pool):
                        ctx.spray_step_device(d_out.data_ptr(), SPRAY, pool.data_ptr(), count, 0, 0, S, K)
                    fn()
                    ctx.synchronize()
                    head = d_out[:8].cpu().numpy().view(np.uint32)
                    variants.append((f"B: {cloud} cloud, {label}", ctx, fn, 1, int(head[0])))
            for v in variants:  # warm-up
                run(v[1], v[2], launches, v[3])
            times = {v[0]: [] for v in variants}
            for _ in range(rounds):  # alternating rounds
                for v in variants:
                    times[v[0]].append(run(v[1], v[2], launches, v[3]))
            a = statistics.median(times[variants[0][0]])
            for v in variants:
                rec = {"particles": count, "substeps": S, "case": v[0], "launches_per_round": launches}
                rec.update(summarize(times[v[0]]))
                if len(v) > 4:
                    rec["survivors"] = v[4]
                    rec["A_over_B"] = round(a / rec["median_us"], 2)
                table.append(rec)
        del pools, d_q, d_rec, d_out
    return table, H


def async_round_trip(ctx, repeats=20):
    """One pool of 65,535 through ocean_spray_step_async: wall clock from the request to the landed copy, and the
    copy's own time."""
    count = oh.SPRAY_MAX_STAGED
    dev = torch.device("cuda", ctx.device)
    pools, _, _, _ = clouds(ctx, count, dev)
    pool = pools["low"].cpu().numpy()
    ctx.set_readback_timing(True)
    slot = oh.PinnedBuffer((count + 1) * 32)
    wall, copy = [], []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.spray_step_async(SPRAY, pool, None, 1, K, buf=slot)
        rb.wait()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
            copy.append(1e3 * rb.copy_ms())
        total = rb.spray()[0]
        rb.release()
    slot.release()
    ctx.set_readback_timing(False)
    return {"particles": count, "survivors": total, "bytes_each_way": (count + 1) * 32,
            "round_trip_us_median": round(statistics.median(wall), 1), "round_trip_us_min": round(min(wall), 1),
            "copy_us_median": round(statistics.median(copy), 1), "requests": repeats}


def markdown(res):
    lines = ["| particles | S | case | kernels (us) | survivors | A / B |", "|---|---|---|---|---|---|"]
    for r in res["kernel"]:
        lines.append(f"| {r['particles']} | {r['substeps']} | {r['case']} | {r['median_us']:.1f} ± {r['spread_us']:.1f} | "
                     f"{r.get('survivors', '—')} | {r.get('A_over_B', '—')} |")
    a = res["async"]
    lines += ["", f"async, {a['particles']} particles, S = 1 ({a['bytes_each_way']} B each way): round trip "
                  f"{a['round_trip_us_median']} us median / {a['round_trip_us_min']} us min, copy {a['copy_us_median']} us"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="calls per round (at least 10)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("spraybench.py needs a GPU: it measures")
    launches, rounds = max(10, args.launches), max(3, args.rounds)
    bodies = {"on": make_body({}), "off": make_body({"OCEAN_RAY_BOUNDS": "0"})}
    try:
        table, H = measure(bodies, launches, rounds)
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures, OCEAN_F_VELOCITY), K = {K}",
               "device": torch.cuda.get_device_name(0), "H": H, "kernel": table,
               "async": async_round_trip(bodies["on"].ctx)}
    finally:
        for wb in bodies.values():
            wb.OnDisable()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
