#!/usr/bin/env python3
"""The ray casts and the surface bounds (csrc/ray.hip, csrc/bounds.hip) at cfg3's shape and parameters: one context
of 4 x 1024^2 with the scene's cascades, full outputs, K = 2, S = 64, B = 8.

    python tools/raybench.py [--rounds 5] [--launches 20] [--markdown]

1. ocean_raycast_device over 65,536 rays (the host forms stop at 16,384), kernel time by events
   (ocean_set_kernel_timing, kind 2), with the air skip on and off (OCEAN_RAY_BOUNDS, two contexts on the same
   frame), alternating rounds: a camera fan from 20 m up, and the same origins pointing straight down, where the
   skip helps least.  The two contexts' results are compared bit for bit first.
2. The formulation a host has without the entry: S + B + 2 launches of ocean_query_surface_device over the same
   number of points, kernel time only (none of its host round trips).
3. ocean_raycast_async over 4,096 rays, wall clock from the call to the landed 128 KiB.
4. The two bounds kernels alone (one ocean_surface_bounds after every step), against the slice bytes of the tile.
Each figure is the median over the rounds with its range.  Prints one JSON line; --markdown appends the tables of
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

N, CASCADES, RAYS, ASYNC_RAYS, K, S, B = 1024, 4, 65536, 4096, 2, 64, 8
vp = ctypes.c_void_p
f32 = np.float32


def make_context(skip):
    os.environ["OCEAN_RAY_BOUNDS"] = "1" if skip else "0"  # read once, in ocean_create
    try:
        wb = oh.scene_water_body(n=N, n_cascades=CASCADES)
        ctx = oh.OceanContext(N, CASCADES, 1, 0)
        ctx.set_params(wb.params(), [c.as_dict() for c in wb.cascades])
        ctx.generate_noise(20251121)
        ctx.init_spectrum()
        for f in range(3):
            ctx.step(f / 60.0)
        ctx.synchronize()
        return ctx
    finally:
        del os.environ["OCEAN_RAY_BOUNDS"]


def summarize(rounds, digits=2):
    return {"median": round(statistics.median(rounds), digits), "min": round(min(rounds), digits),
            "max": round(max(rounds), digits), "rounds": [round(r, digits) for r in rounds]}


def camera_fan(count, down=False):
    """count rays from (0, 20, 0): a fan of 90 degrees in yaw and 2 to 60 degrees below the horizon, searched over
    2000 m; `down`: the same count straight down from origins spread over the patch, searched over 40 m."""
    side = int(round(count ** 0.5))
    assert side * side == count
    r = np.zeros((count, 8), f32)
    if down:
        xs = np.linspace(-1000.0, 1000.0, side)
        gx, gz = np.meshgrid(xs, xs)
        r[:, 0], r[:, 1], r[:, 2], r[:, 4], r[:, 7] = gx.ravel(), 20.0, gz.ravel(), -1.0, 40.0
        return r
    yaw, pitch = np.meshgrid(np.radians(np.linspace(-45.0, 45.0, side)), np.radians(np.linspace(-2.0, -60.0, side)))
    r[:, 1] = 20.0
    r[:, 3] = (np.cos(pitch) * np.sin(yaw)).ravel()
    r[:, 4] = np.sin(pitch).ravel()
    r[:, 5] = (np.cos(pitch) * np.cos(yaw)).ravel()
    r[:, 7] = 2000.0
    return r


def timed_kind2(ctx, fn, launches):
    """us per launch of `fn`, kernel time by events; one untimed call first (it also brings the bounds up to date)."""
    oh._check(fn(), "launch")
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(launches):
        oh._check(fn(), "launch")
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == launches, (cnt, launches)
    return 1e3 * ms / cnt


def ray_table(on, off, rays, launches, rounds):
    dev = torch.device("cuda", on.device)
    d_rays = torch.from_numpy(rays).to(dev)
    outs = {"on": torch.empty(len(rays) * 8, dtype=torch.float32, device=dev),
            "off": torch.empty(len(rays) * 8, dtype=torch.float32, device=dev)}
    torch.cuda.synchronize()
    variants = [(label, ctx, (lambda ctx=ctx, label=label: ctx.lib.ocean_raycast_device(
        ctx._h, 0, K, S, B, vp(d_rays.data_ptr()), len(rays), vp(outs[label].data_ptr()))))
        for label, ctx in (("on", on), ("off", off))]
    times = {label: [] for label, _, _ in variants}
    for _ in range(rounds):
        for label, ctx, fn in variants:
            times[label].append(timed_kind2(ctx, fn, launches))
    torch.cuda.synchronize()
    assert torch.equal(outs["on"], outs["off"])  # the skip changes no bit
    status = outs["on"].view(-1, 8)[:, 3].cpu().numpy()
    res = {label: summarize(v) for label, v in times.items()}
    res["rays"] = len(rays)
    res["status_share"] = {name: round(float((status == s).mean()), 3)
                           for s, name in ((oh.RAY_MISS, "miss"), (oh.RAY_HIT, "hit"), (oh.RAY_SUBMERGED, "submerged"))}
    res["off_over_on"] = round(res["off"]["median"] / res["on"]["median"], 2)
    return res


def query_formulation(ctx, launches, rounds):
    """S + B + 2 launches of ocean_query_surface_device over RAYS points: us for all of them together."""
    dev = torch.device("cuda", ctx.device)
    rng = np.random.default_rng(20251121)
    d_q = torch.from_numpy(rng.uniform(-2000.0, 2000.0, (RAYS, 2)).astype(f32)).to(dev)
    out = torch.empty(RAYS * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def fn():
        return ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, K, vp(d_q.data_ptr()), RAYS,
                                                  vp(out.data_ptr()))
    per = [timed_kind2(ctx, fn, launches) for _ in range(rounds)]
    res = summarize([p * (S + B + 2) for p in per])
    res["launches_of_the_formulation"], res["one_query_launch_us"] = S + B + 2, summarize(per)
    return res


def async_table(ctx, rounds):
    rays = camera_fan(ASYNC_RAYS)
    slot = oh.PinnedBuffer(ASYNC_RAYS * 32)
    ms = []
    for r in range(rounds + 1):
        ctx.synchronize()
        t0 = time.perf_counter()
        rb = ctx.raycast_async(rays, iterations=K, steps=S, refine=B, buf=slot)
        rb.wait()
        dt = 1e3 * (time.perf_counter() - t0)
        rb.release()
        if r:  # the first request creates the slot
            ms.append(dt)
    slot.release()
    res = summarize(ms, 3)
    res["rays"], res["bytes_landed"] = ASYNC_RAYS, ASYNC_RAYS * 32
    return res


def bounds_table(ctx, launches, rounds):
    us = []
    for _ in range(rounds):
        ctx.synchronize()
        ctx.set_kernel_timing(True)
        ctx.kernel_stats(2)
        for f in range(launches):
            ctx.step(1.0 + f / 60.0)  # drops the cached bounds
            ctx.surface_bounds()
        ms, cnt = ctx.kernel_stats(2)
        ctx.set_kernel_timing(False)
        assert cnt == launches, (cnt, launches)
        us.append(1e3 * ms / cnt)
    res = summarize(us)
    res["slice_bytes_of_the_tile"] = CASCADES * N * N * 16
    res["gb_per_s"] = round(res["slice_bytes_of_the_tile"] / (res["median"] * 1e-6) / 1e9, 1)
    return res


def markdown(res):
    lines = ["| 65,536 rays, K = 2, S = 64, B = 8 (kernel, us: median [min, max]) | skip on | skip off | off / on |",
             "|---|---|---|---|"]
    for key, label in (("fan", "camera fan from 20 m"), ("down", "straight down")):
        t = res[key]
        lines.append(f"| {label} | {t['on']['median']} [{t['on']['min']}, {t['on']['max']}] | "
                     f"{t['off']['median']} [{t['off']['min']}, {t['off']['max']}] | {t['off_over_on']} |")
    q, a, b = res["query_formulation"], res["async"], res["bounds"]
    lines += ["", "| | |", "|---|---|",
              f"| {q['launches_of_the_formulation']} launches of ocean_query_surface_device, 65,536 points (us) | "
              f"{q['median']} [{q['min']}, {q['max']}] |",
              f"| ocean_raycast_async, {a['rays']} rays, call to landed {a['bytes_landed'] // 1024} KiB (ms) | "
              f"{a['median']} [{a['min']}, {a['max']}] |",
              f"| the two bounds kernels, {b['slice_bytes_of_the_tile'] >> 20} MiB of slices (us) | "
              f"{b['median']} [{b['min']}, {b['max']}], {b['gb_per_s']} GB/s |"]
    return "\n".join(lines)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=20, help="launches per round (at least 20)")
    ap.add_argument("--markdown", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("raybench.py needs a GPU: it measures")
    rounds, launches = max(3, args.rounds), max(20, args.launches)
    on, off = make_context(True), make_context(False)
    try:
        res = {"workload": f"{CASCADES} x {N}^2 (cfg3 shape and parameters), full outputs; K = {K}, S = {S}, B = {B}",
               "device": torch.cuda.get_device_name(0), "rounds": rounds, "launches_per_round": launches,
               "bounds_records": on.surface_bounds().tolist(),
               "fan": ray_table(on, off, camera_fan(RAYS), launches, rounds),
               "down": ray_table(on, off, camera_fan(RAYS, down=True), launches, rounds),
               "query_formulation": query_formulation(on, launches, rounds),
               "async": async_table(on, rounds),
               "bounds": bounds_table(off, launches, rounds)}
    finally:
        on.close()
        off.close()
    print(json.dumps(res))
    if args.markdown:
        print(markdown(res))


if __name__ == "__main__":
    main()
