#!/usr/bin/env python3
"""The whitecap emitters (ocean_whitecaps_device, csrc/whitecaps.hip) against what a host does today for the same
answer, at cfg3's textures: one velocity context of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/whitecapbench.py [--launches 20] [--rounds 3] [--markdown]

A is today's path: ocean_surface_grid_device in OCEAN_GRID_VERTICES mode over the same 1024 x 1024 nodes (one
texel of the finest cascade apart), whose 32 B per node, 32 MiB, the host then lands and thresholds on the CPU;
the landing is priced at the README's measured link rate (LINK_GBPS), not run.  B is the three whitecap launches
(count, scan, emit) at the thresholds that select about 0.1 %, 1 % and 10 % of the nodes -- quantiles of the foam
column of A's own result -- with a capacity of twice the list (at most OCEAN_WHITECAP_MAX_RECORDS), whose
(capacity + 1) x 32 B the host lands instead.  Also all nodes (threshold below every foam) and none (above).

Prediction, written before the first run: count reads the TURB taps alone (a quarter of A's texture reads, no
DERIV, no normal, no 32 B store per node) and emit touches only the selected lanes, so B should cost a fraction of
A that grows with the selected share; the scan is one small workgroup.

Time is the kernels' own (ocean_set_kernel_timing / ocean_kernel_stats kind 2: events on the dispatches, from the
start of count to the end of emit).  After a warm-up of every variant, `rounds` alternating rounds of `launches`
back-to-back calls each; a round's figure is its mean per call, the reported figure the median over the rounds,
the spread max - min over the rounds.  Also the round trip of one list through ocean_whitecaps_async (request to
landed, wall clock, and the copy's own time).  Prints one JSON line; --markdown appends the table of
docs/MEASUREMENTS.md.  A record, not a gate."""
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

N, CASCADES, NODES = 1024, 4, 1024
ORIGIN = (-311.3, 127.9)
SHARES = (0.001, 0.01, 0.1)
LINK_GBPS = 51.0  # README: the device-to-host copy of the RGBA readback loop
vp = ctypes.c_void_p


def run(ctx, fn, launches):
    """Mean kernel time per call in us over `launches` back-to-back calls, and the last kernel's symbol."""
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


def link_us(nbytes):
    return round(nbytes / (LINK_GBPS * 1e3), 1)


def measure(wb, launches, rounds):
    ctx = wb.ctx
    dev = torch.device("cuda", ctx.device)
    texel = min(c.wavelength for c in wb.cascades) / N
    g = (ORIGIN[0], ORIGIN[1], texel, texel, NODES, NODES)
    m = NODES * NODES
    out_a = torch.empty(m * 8, dtype=torch.float32, device=dev)
    out_b = torch.empty((oh.WHITECAP_MAX_RECORDS + 1) * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def grid_fn():
        return ctx.lib.ocean_surface_grid_device(ctx._h, 0, oh.GRID_VERTICES, 0, 0.0, *g, vp(out_a.data_ptr()), m * 32)

    oh._check(grid_fn(), "ocean_surface_grid_device")
    ctx.synchronize()
    vertices = out_a.cpu().numpy().reshape(m, 8)
    foam = vertices[:, 3]
    cases = [("all", float(foam.min()) - 1.0), ("none", float(foam.max()) + 1.0)]
    positive = foam[foam > 0]
    assert len(positive), "the scene has no foam"
    for s in SHARES:  # (where fewer nodes than that carry foam: all that do; the record holds the share selected)
        th = float(np.quantile(foam, 1.0 - s).astype(np.float32))
        cases.append((f"{100 * s:g}%", th if th > 0 else float(positive.min())))

    variants = [("A", grid_fn, None, m * 32)]
    for name, th in cases:
        total = int((foam >= np.float32(th)).sum())
        cap = min(max(2 * total, 256), oh.WHITECAP_MAX_RECORDS)

        def fn(th=th, cap=cap):
            return ctx.lib.ocean_whitecaps_device(ctx._h, 0, 0.0, th, *g, cap, vp(out_b.data_ptr()), (cap + 1) * 32)

        # the list is the grid's own vertices above the threshold, in node order
        oh._check(fn(), "ocean_whitecaps_device")
        ctx.synchronize()
        got_total, rec = oh.OceanContext.parse_whitecaps(out_b.cpu().numpy()[:(cap + 1) * 8])
        idx = np.flatnonzero(foam >= np.float32(th))
        assert got_total == total == len(idx), (name, got_total, total)
        assert np.array_equal(rec[:, :4], vertices[idx[:len(rec)], :4]), name
        variants.append((name, fn, {"threshold": th, "selected": total, "share": round(total / m, 5), "capacity": cap,
                                    "written": len(rec)}, (cap + 1) * 32))
    for _, fn, _, _ in variants:  # warm-up
        run(ctx, fn, launches)
    times, symbols = {v[0]: [] for v in variants}, {}
    for _ in range(rounds):  # alternating rounds
        for label, fn, _, _ in variants:
            us, symbols[label] = run(ctx, fn, launches)
            times[label].append(us)
    table = []
    for label, _, info, nbytes in variants:
        rec = {"case": label, "nodes": m, "launches_per_round": launches, "bytes_landed": nbytes,
               "link_us_at_%g_GBps" % LINK_GBPS: link_us(nbytes), "symbol": symbols[label]}
        rec.update(summarize(times[label]))
        rec.update(info or {})
        rec["kernel_plus_link_us"] = round(rec["median_us"] + link_us(nbytes), 1)
        table.append(rec)
    a = table[0]
    for rec in table[1:]:
        rec["kernel_ratio_A_over_B"] = round(a["median_us"] / rec["median_us"], 2)
        rec["total_ratio_A_over_B"] = round(a["kernel_plus_link_us"] / rec["kernel_plus_link_us"], 2)
    return g, cases, table


def async_round_trip(ctx, g, threshold, capacity, repeats=20):
    """One list through ocean_whitecaps_async: wall clock from the request to the landed copy, and the copy's own time."""
    ctx.set_readback_timing(True)
    slot = oh.PinnedBuffer((capacity + 1) * 32)
    wall, copy = [], []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.whitecaps_async(threshold, *g, capacity=capacity, buf=slot)
        rb.wait()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
            copy.append(1e3 * rb.copy_ms())
        total = rb.whitecaps()[0]
        rb.release()
    slot.release()
    ctx.set_readback_timing(False)
    return {"threshold": threshold, "capacity": capacity, "selected": total, "bytes": (capacity + 1) * 32,
            "round_trip_us_median": round(statistics.median(wall), 1), "round_trip_us_min": round(min(wall), 1),
            "copy_us_median": round(statistics.median(copy), 1), "requests": repeats}


def markdown(res):
    lines = ["| case | selected (share) | capacity | kernels (us) | bytes landed | link at %g GB/s (us) | kernels + link (us) |"
             % LINK_GBPS, "|---|---|---|---|---|---|---|"]
    for r in res["kernel"]:
        sel = f"{r['selected']} ({100 * r['share']:.3g} %)" if "selected" in r else "every node, 32 B each"
        key = "link_us_at_%g_GBps" % LINK_GBPS
        lines.append(f"| {r['case']} | {sel} | {r.get('capacity', '—')} | {r['median_us']:.1f} ± {r['spread_us']:.1f} | "
                     f"{r['bytes_landed']} | {r[key]} | {r['kernel_plus_link_us']} |")
    a = res["async"]
    lines += ["", f"async, {a['selected']} selected, capacity {a['capacity']} ({a['bytes']} B): round trip "
                  f"{a['round_trip_us_median']} us median / {a['round_trip_us_min']} us min, copy {a['copy_us_median']} us"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="calls per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("whitecapbench.py needs a GPU: it measures")
    launches, rounds = max(20, args.launches), max(3, args.rounds)
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, velocity=True, readback="height").Awake()
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    try:
        g, cases, table = measure(wb, launches, rounds)
        one_percent = dict(cases)["1%"]
        sel = next(r["selected"] for r in table if r["case"] == "1%")
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures, OCEAN_F_VELOCITY), {NODES} x {NODES} nodes",
               "device": torch.cuda.get_device_name(0), "link_GBps": LINK_GBPS, "kernel": table,
               "async": async_round_trip(wb.ctx, g, one_percent, min(max(2 * sel, 256), oh.WHITECAP_MAX_RECORDS))}
    finally:
        wb.OnDisable()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
