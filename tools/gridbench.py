#!/usr/bin/env python3
"""The grid kernel (ocean_surface_grid_device, csrc/grid.hip) against the point-list entries over the same
nodes, at cfg3's textures: one context of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/gridbench.py [--launches 20] [--rounds 3] [--markdown]

A is the point-list path over OceanContext.grid_points(...) uploaded once: ocean_query_surface_device at
K = 4 (for GRID_SURFACE) and ocean_sample_world_device at lod 0 (for GRID_VERTICES).  B is the grid kernel
with each workgroup tile: 64 x 4 (a strip), 32 x 8 and 16 x 16 (OCEAN_GRID_TILE = 64 / 32 / 16; one context
per shape, since the knob is read in ocean_create; the contexts hold the same textures bit for bit).
GRID_HEIGHTFIELD at K = 4 is timed beside them; it has no point-list counterpart of its size.

Grids: 1024 x 1024 nodes at 1, 0.25 and 4 texels of the finest cascade.  Time is the kernels' own
(ocean_set_kernel_timing / ocean_kernel_stats kind 2: events on the dispatch itself).  After a warm-up of
every variant, `rounds` alternating rounds A, B64, B32, B16 of `launches` back-to-back launches each; a
round's figure is its mean per launch, the reported figure the median over the rounds, the spread max - min
over the rounds.  B is "no slower" when its median does not exceed A's by more than the larger of the two
spreads.  Also: the round trip of a 256 x 256 grid through ocean_surface_grid_async in GRID_HEIGHTFIELD and
GRID_SURFACE mode (request to landed, wall clock, and the copy's own time from ocean_readback_copy_ms).
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

N, CASCADES, NODES = 1024, 4, 1024
SHAPES = ((64, "64x4"), (32, "32x8"), (16, "16x16"))
SPACINGS = (1.0, 0.25, 4.0)  # texels of the finest cascade
ORIGIN = (-311.3, 127.9)
K = 4
vp = ctypes.c_void_p


def make_ctx(tile_w):
    os.environ["OCEAN_GRID_TILE"] = str(tile_w)
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, readback="height").Awake()
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    return wb


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


def kernel_table(wbs, launches, rounds):
    base = wbs[SHAPES[0][0]].ctx  # A runs on the first context: the textures are the same in all three
    dev = torch.device("cuda", base.device)
    texel = min(c.wavelength for c in wbs[SHAPES[0][0]].cascades) / N
    out_a = torch.empty(NODES * NODES * 12, dtype=torch.float32, device=dev)
    out_b = torch.empty(NODES * NODES * 8, dtype=torch.float32, device=dev)
    table = []
    for sp in SPACINGS:
        g = (ORIGIN[0], ORIGIN[1], sp * texel, sp * texel, NODES, NODES)
        q = oh.OceanContext.grid_points(*g)
        p2 = torch.from_numpy(q).to(dev)
        p3 = torch.from_numpy(np.concatenate([q, np.zeros((len(q), 1), np.float32)], axis=1)).to(dev)
        torch.cuda.synchronize()
        m = len(q)

        def grid_fn(ctx, mode, it):
            nbytes = m * (4 if mode == oh.GRID_HEIGHTFIELD else 32)
            return lambda: ctx.lib.ocean_surface_grid_device(ctx._h, 0, mode, it, 0.0, *g[:4], NODES, NODES,
                                                             vp(out_b.data_ptr()), nbytes)

        cases = {
            "surface_k4": (lambda: base.lib.ocean_query_surface_device(base._h, 0, oh.QUERY_SURFACE, K, vp(p2.data_ptr()),
                                                                       m, vp(out_a.data_ptr())),
                           oh.GRID_SURFACE, K),
            "vertices_lod0": (lambda: base.lib.ocean_sample_world_device(base._h, 0, vp(p3.data_ptr()), m,
                                                                         vp(out_a.data_ptr())),
                              oh.GRID_VERTICES, 0),
            "heightfield_k4": (None, oh.GRID_HEIGHTFIELD, K),
        }
        for name, (a_fn, mode, it) in cases.items():
            variants = ([("A", base, a_fn)] if a_fn else []) + \
                       [(label, wbs[tw].ctx, grid_fn(wbs[tw].ctx, mode, it)) for tw, label in SHAPES]
            for _, ctx, fn in variants:  # warm-up
                run(ctx, fn, launches)
                if name == "surface_k4" and fn is not a_fn:  # the same records as the point list, bit for bit
                    torch.cuda.synchronize()
                    assert torch.equal(out_a[:m * 8], out_b[:m * 8]), f"grid kernel differs from the point query at {sp} texels"
            times = {label: [] for label, _, _ in variants}
            symbols = {}
            for _ in range(rounds):  # alternating rounds
                for label, ctx, fn in variants:
                    us, symbols[label] = run(ctx, fn, launches)
                    times[label].append(us)
            rec = {"grid_texels": sp, "case": name, "nodes": m, "launches_per_round": launches}
            for label in times:
                rec[label] = summarize(times[label])
                rec[label]["symbol"] = symbols[label]
            if a_fn:
                a = rec["A"]
                for _, label in SHAPES:
                    b = rec[label]
                    b["no_slower_than_A"] = b["median_us"] <= a["median_us"] + max(a["spread_us"], b["spread_us"])
                    b["ratio_A_over_B"] = round(a["median_us"] / b["median_us"], 3)
            table.append(rec)
    return table


def async_round_trips(wb, repeats=20):
    """256 x 256 nodes at one texel of the finest cascade through ocean_surface_grid_async, with the library's
    default tile: wall clock from the request to the landed copy, and the copy's own time."""
    ctx = wb.ctx
    texel = min(c.wavelength for c in wb.cascades) / N
    g = (ORIGIN[0], ORIGIN[1], texel, texel, 256, 256)
    ctx.set_readback_timing(True)
    out = {}
    for name, mode in (("heightfield", oh.GRID_HEIGHTFIELD), ("surface", oh.GRID_SURFACE)):
        nbytes = 256 * 256 * (4 if mode == oh.GRID_HEIGHTFIELD else 32)
        slot = oh.PinnedBuffer(nbytes)
        wall, copy = [], []
        for i in range(repeats + 5):
            ctx.synchronize()
            t0 = time.perf_counter()
            rb = ctx.surface_grid_async(*g, mode=mode, iterations=K, buf=slot)
            rb.wait()
            t1 = time.perf_counter()
            if i >= 5:
                wall.append(1e6 * (t1 - t0))
                copy.append(1e3 * rb.copy_ms())
            rb.release()
        slot.release()
        out[name] = {"bytes": nbytes, "round_trip_us_median": round(statistics.median(wall), 1),
                     "round_trip_us_min": round(min(wall), 1), "copy_us_median": round(statistics.median(copy), 1),
                     "requests": repeats}
    ctx.set_readback_timing(False)
    return out


def markdown(res):
    lines = ["| grid (texels) | case | A point list (us) | 64x4 (us) | 32x8 (us) | 16x16 (us) |", "|---|---|---|---|---|---|"]

    def cell(r):
        return f"{r['median_us']:.1f} ± {r['spread_us']:.1f}" if r else "—"
    for rec in res["kernel"]:
        lines.append(f"| {rec['grid_texels']} | {rec['case']} | {cell(rec.get('A'))} | " +
                     " | ".join(cell(rec[label]) for _, label in SHAPES) + " |")
    lines.append("")
    lines.append("| 256 x 256 async | bytes | round trip median / min (us) | copy median (us) |")
    lines.append("|---|---|---|---|")
    for name, r in res["async_256x256"].items():
        lines.append(f"| {name} | {r['bytes']} | {r['round_trip_us_median']} / {r['round_trip_us_min']} | {r['copy_us_median']} |")
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--launches", type=int, default=20, help="launches per round (at least 20)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("gridbench.py needs a GPU: it measures")
    launches, rounds = max(20, args.launches), max(3, args.rounds)
    wbs = {tw: make_ctx(tw) for tw, _ in SHAPES}
    os.environ.pop("OCEAN_GRID_TILE", None)
    default = make_ctx(0)  # 0 is no shape: the library's kept default
    os.environ.pop("OCEAN_GRID_TILE", None)
    try:
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures), {NODES} x {NODES} nodes, K = {K}",
               "device": torch.cuda.get_device_name(0), "kernel": kernel_table(wbs, launches, rounds),
               "async_256x256": async_round_trips(default)}
    finally:
        for wb in list(wbs.values()) + [default]:
            wb.OnDisable()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
