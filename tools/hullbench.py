#!/usr/bin/env python3
"""The mesh-hull kernel (ocean_body_hydrostatics_device, csrc/hull.hip) against the two things a host does today for
the same hulls, at cfg3's textures: one context of 4 x 1024^2 with the scene's cascades, stepped twice.

    python tools/hullbench.py [--launches 20] [--rounds 3] [--markdown]

M = 4096 bodies with random poses (unit quaternions, scales in [0.5, 3], origins within +-2000 m, cy within +-1 m) share
OceanContext.box_mesh hulls of V = 8, 218 and 1538 vertices (12, 432 and 3072 triangles); K = 4.  At V = 1538 the
existing limit count * nverts <= OCEAN_BODY_MAX_SAMPLES allows 2727 bodies, and that many are run; the table also gives
the time per body.  H is the hull kernel.  A is ocean_query_surface_device over the same M x V world positions of the
vertices, formed on the host in fp32 with ocean.h's formulas and uploaded once: the same lookups, after which the host
still has M x V x 32 B to read back, the clip and the sums to do.  B is ocean_body_buoyancy_device with P = V probes
at the vertices (h = 1, v = 1 / V): the same lookups reduced per body, without clip, area or horizontal force.

Time is the kernels' own (ocean_set_kernel_timing / ocean_kernel_stats kind 2: events on the dispatch itself).  After a
warm-up of all three, `rounds` alternating rounds A, B, H of `launches` back-to-back launches each; a round's figure is
its mean per launch, the reported figure the median over the rounds, the spread max - min over the rounds.  During the
warm-up the worst residual of every body in H is compared with the largest residual of its vertices in A's records and
with B's: the same lookups at the same positions.  Also: the round trip of 4096 bodies of the 218-vertex hull through
ocean_body_hydrostatics_async (call to landed data, wall clock, and the copy's own time from ocean_readback_copy_ms).
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from bodybench import probe_positions, random_bodies, run, summarize  # noqa: E402

N, CASCADES, BODIES, K = 1024, 4, 4096, 4
HULLS = ((1, 1, 1), (6, 6, 6), (16, 16, 16))  # box_mesh cells: V = 8, 218, 1538
vp = ctypes.c_void_p
f32 = np.float32


def kernel_table(ctx, launches, rounds):
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    all_bodies = random_bodies(rng, BODIES)
    table = []
    for cells in HULLS:
        verts, tris = oh.OceanContext.box_mesh(1.0, 1.0, 1.0, *cells)
        nv, nt = len(verts), len(tris)
        count = min(BODIES, oh.BODY_MAX_SAMPLES // nv)
        bodies = all_bodies[:count]
        hull = np.concatenate([verts, np.ones((nv, 1), f32), np.full((nv, 1), 1.0 / nv, f32)], axis=1)
        q = probe_positions(hull, bodies)
        m = len(q)
        d_bodies = torch.from_numpy(np.ascontiguousarray(bodies)).to(dev)
        d_verts, d_tris = torch.from_numpy(verts).to(dev), torch.from_numpy(tris).to(dev)
        d_hull, d_q = torch.from_numpy(hull).to(dev), torch.from_numpy(q).to(dev)
        out_a = torch.empty(m * 8, dtype=torch.float32, device=dev)
        out_b = torch.empty(count * 8, dtype=torch.float32, device=dev)
        out_h = torch.empty(count * 16, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        variants = (
            ("A", lambda: ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), m,
                                                             vp(out_a.data_ptr()))),
            ("B", lambda: ctx.lib.ocean_body_buoyancy_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_hull.data_ptr()), nv,
                                                             vp(d_bodies.data_ptr()), count, vp(out_b.data_ptr()))),
            ("H", lambda: ctx.lib.ocean_body_hydrostatics_device(ctx._h, 0, K, vp(d_verts.data_ptr()), nv,
                                                                 vp(d_tris.data_ptr()), nt, vp(d_bodies.data_ptr()), count,
                                                                 vp(out_h.data_ptr()))),
        )
        for _, fn in variants:  # warm-up
            run(ctx, fn, launches)
        torch.cuda.synchronize()
        worst = out_a.view(count, nv, 8)[:, :, 3].max(dim=1).values
        assert torch.equal(worst, out_h.view(count, 16)[:, 7]) and torch.equal(worst, out_b.view(count, 8)[:, 7]), nv
        times, symbols = {"A": [], "B": [], "H": []}, {}
        for _ in range(rounds):  # alternating rounds
            for label, fn in variants:
                us, symbols[label] = run(ctx, fn, launches)
                times[label].append(us)
        rec = {"vertices": nv, "triangles": nt, "bodies": count, "samples": m, "launches_per_round": launches}
        for label in times:
            rec[label] = summarize(times[label])
            rec[label]["symbol"] = symbols[label]
        h = rec["H"]
        h["ns_per_body"] = round(1e3 * h["median_us"] / count, 2)
        h["ratio_A_over_H"] = round(rec["A"]["median_us"] / h["median_us"], 3)
        h["ratio_B_over_H"] = round(rec["B"]["median_us"] / h["median_us"], 3)
        table.append(rec)
    return table


def async_round_trip(ctx, repeats=20):
    """4096 bodies of the 218-vertex hull through ocean_body_hydrostatics_async: 160 KiB of bodies, 2.6 KiB of vertices
    and 5.1 KiB of indices up, 256 KiB down; wall clock from the call to the landed copy, and the copy's own time."""
    rng = np.random.default_rng(7)
    verts, tris = oh.OceanContext.box_mesh(1.0, 1.0, 1.0, *HULLS[1])
    bodies = random_bodies(rng, BODIES)
    ctx.set_readback_timing(True)
    slot = oh.PinnedBuffer(len(bodies) * 64)
    wall, copy = [], []
    for i in range(repeats + 5):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.body_hydrostatics_async(verts, tris, bodies, iterations=K, buf=slot)
        rb.wait()
        t1 = time.perf_counter()
        if i >= 5:
            wall.append(1e6 * (t1 - t0))
            copy.append(1e3 * rb.copy_ms())
        rb.release()
    slot.release()
    ctx.set_readback_timing(False)
    return {"bodies": len(bodies), "vertices": len(verts), "triangles": len(tris),
            "bytes_up": bodies.nbytes + verts.nbytes + tris.nbytes, "bytes_down": len(bodies) * 64,
            "round_trip_us_median": round(statistics.median(wall), 1), "round_trip_us_min": round(min(wall), 1),
            "copy_us_median": round(statistics.median(copy), 1), "requests": repeats}


def markdown(res):
    lines = ["| V / T | bodies | samples | A point query (us) | B probe bodies (us) | H hull kernel (us) | A / H | B / H | "
             "H per body (ns) |", "|---|---|---|---|---|---|---|---|---|"]
    for rec in res["kernel"]:
        a, b, h = rec["A"], rec["B"], rec["H"]
        lines.append(f"| {rec['vertices']} / {rec['triangles']} | {rec['bodies']} | {rec['samples']} | "
                     f"{a['median_us']:.1f} ± {a['spread_us']:.1f} | {b['median_us']:.1f} ± {b['spread_us']:.1f} | "
                     f"{h['median_us']:.1f} ± {h['spread_us']:.1f} | {h['ratio_A_over_H']} | {h['ratio_B_over_H']} | "
                     f"{h['ns_per_body']} |")
    r = res["async_4096x218"]
    lines += ["", "| 4096 x 218 async | bytes up / down | round trip median / min (us) | copy median (us) |", "|---|---|---|---|",
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
        sys.exit("hullbench.py needs a GPU: it measures")
    launches, rounds = max(20, args.launches), max(3, args.rounds)
    wb = oh.scene_water_body(n=N, n_cascades=CASCADES, seed=20251121, mips=False, readback="height").Awake()
    wb.ctx.step(0.5)
    wb.ctx.step(1.0)
    wb.ctx.synchronize()
    try:
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 textures), up to {BODIES} bodies, K = {K}",
               "device": torch.cuda.get_device_name(0), "kernel": kernel_table(wb.ctx, launches, rounds),
               "async_4096x218": async_round_trip(wb.ctx)}
    finally:
        wb.OnDisable()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
