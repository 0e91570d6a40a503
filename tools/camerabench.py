#!/usr/bin/env python3
"""The camera views (csrc/view.hip) at cfg3's shape and parameters: one context of 4 x 1024^2 with the scene's
cascades, full outputs, K = 2, S = 64, B = 8, a 1024 x 1024 image.

    python tools/camerabench.py [--rounds 5] [--launches 10] [--markdown]

1. ocean_camera_device in the three modes, kernel time by events (ocean_set_kernel_timing, kind 2), from a horizon
   camera (20 m up, pitched 10 degrees down, searched over 2000 m) and from a straight-down camera (20 m up,
   searched over 40 m, where the air skip helps least), with the air skip on and off (OCEAN_RAY_BOUNDS) and with the
   row-linear mapping of pixels to lanes (OCEAN_CAMERA_TILE=0): three contexts on the same frame, alternating
   rounds.  The three contexts' images are compared bit for bit first.
2. The yardstick: ocean_raycast_device over the same 2^20 rays, which a host would have built and uploaded (4
   launches of 2^18 rays: count * steps <= OCEAN_RAY_MAX_SAMPLES), kernel time only; its records are compared with
   the HITS image bit for bit.
3. The bytes each form lands per image.
Each figure is the median over the rounds with its range.  Prints one JSON line; --markdown appends the table of
docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402

N, CASCADES, W, H, K, S, B = 1024, 4, 1024, 1024, 2, 64, 8
MODES = (("hits", oh.CAMERA_HITS, 8), ("range", oh.CAMERA_RANGE, 1), ("color", oh.CAMERA_COLOR, 4))
vp = ctypes.c_void_p
f32 = np.float32


def make_context(env):
    os.environ.update(env)  # read once, in ocean_create
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
        for k in env:
            del os.environ[k]


def summarize(rounds, digits=1):
    return {"median": round(statistics.median(rounds), digits), "min": round(min(rounds), digits),
            "max": round(max(rounds), digits)}


def cameras():
    horizon = oh.look_at_camera((0.0, 20.0, 0.0), (60.0, 20.0 - 100.0 * np.tan(np.radians(10.0)), 80.0), (0, 1, 0),
                                0.9, W, H, 0.0, 2000.0)
    down = oh.look_at_camera((0.0, 20.0, 0.0), (0.0, 0.0, 0.0), (0, 0, 1), 0.9, W, H, 0.0, 40.0)
    return (("horizon", horizon), ("down", down))


def pixel_rays(cam):
    """The rays of ocean.h's pixels in fp32, as the kernel forms them: [H * W][8]."""
    fi = np.tile(np.arange(W, dtype=f32), H)[:, None]
    fj = np.repeat(np.arange(H, dtype=f32), W)[:, None]
    raw = (cam[None, 3:6] + fi * cam[None, 6:9]) + fj * cam[None, 9:12]
    ln = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    rays = np.empty((W * H, 8), f32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = cam[0:3], raw / ln[:, None], cam[12], cam[13]
    return rays


def timed_kind2(ctx, fn, launches, per_call=1):
    """us per call of `fn` (per_call launches each), kernel time by events; one untimed call first."""
    fn()
    ctx.synchronize()
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    for _ in range(launches):
        fn()
    ms, cnt = ctx.kernel_stats(2)
    ctx.set_kernel_timing(False)
    assert cnt == launches * per_call, (cnt, launches, per_call)
    return 1e3 * ms / launches


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "camerabench needs a GPU"
    ctxs = {"skip": make_context({"OCEAN_RAY_BOUNDS": "1"}), "noskip": make_context({"OCEAN_RAY_BOUNDS": "0"}),
            "rowlinear": make_context({"OCEAN_CAMERA_TILE": "0"})}
    dev = torch.device("cuda", ctxs["skip"].device)
    mat = oh.material(roughness=0.3, lod_slope=0.004)
    out = {k: torch.empty(W * H * 8, dtype=torch.float32, device=dev) for k in ctxs}
    d_rays = torch.empty(W * H * 8, dtype=torch.float32, device=dev)
    d_rec = torch.empty(W * H * 8, dtype=torch.float32, device=dev)
    res = {"n": N, "cascades": CASCADES, "width": W, "height": H, "k": K, "steps": S, "refine": B, "cameras": {}}
    for cname, cam in cameras():
        entry = {}
        for mname, mode, per in MODES:
            nbytes = W * H * per * 4
            fns = {k: (lambda c=c, k=k: oh._check(c.lib.ocean_camera_device(
                c._h, 0, mode, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(out[k].data_ptr()), nbytes),
                "ocean_camera_device")) for k, c in ctxs.items()}
            times = {k: [] for k in ctxs}
            for _ in range(a.rounds):
                for k, c in ctxs.items():
                    times[k].append(timed_kind2(c, fns[k], a.launches))
            torch.cuda.synchronize()
            n = W * H * per
            assert torch.equal(out["skip"][:n].view(torch.int32), out["noskip"][:n].view(torch.int32))
            assert torch.equal(out["skip"][:n].view(torch.int32), out["rowlinear"][:n].view(torch.int32))
            entry[mname] = {k: summarize(v) for k, v in times.items()}
            entry[mname]["bytes"] = nbytes
            if mode == oh.CAMERA_HITS:
                status = out["skip"][:n].view(-1, 8)[:, 3].cpu().numpy()
                entry["status_share"] = {name: round(float((status == s).mean()), 3) for s, name in
                                         ((oh.RAY_MISS, "miss"), (oh.RAY_HIT, "hit"), (oh.RAY_SUBMERGED, "submerged"))}
                hits = out["skip"][:n].clone()
        # the yardstick: the same rays through ocean_raycast_device, 4 launches of 2^18
        d_rays.copy_(torch.from_numpy(pixel_rays(cam).ravel()).to(dev))
        torch.cuda.synchronize()
        part = W * H // 4
        assert part * S <= oh.RAY_MAX_SAMPLES
        ray_times = {}
        for k in ("skip", "noskip"):
            c = ctxs[k]

            def cast(c=c):
                for q in range(4):
                    oh._check(c.lib.ocean_raycast_device(c._h, 0, K, S, B, vp(d_rays.data_ptr() + q * part * 32), part,
                                                         vp(d_rec.data_ptr() + q * part * 32)), "ocean_raycast_device")
            ray_times[k] = summarize([timed_kind2(c, cast, a.launches, 4) for _ in range(a.rounds)])
        torch.cuda.synchronize()
        assert torch.equal(d_rec.view(torch.int32), hits.view(torch.int32))  # the shared march: bit for bit
        entry["raycast_device"] = ray_times
        entry["raycast_device"]["bytes_up_and_down"] = 2 * W * H * 32
        res["cameras"][cname] = entry
    for c in ctxs.values():
        c.close()
    print(json.dumps(res))
    if a.markdown:
        print("\n| camera | mode | air skip on, 8 x 8 tiles (us) | skip off (us) | skip on, row-linear (us) | bytes landed |")
        print("|---|---|---|---|---|---|")
        for cname, e in res["cameras"].items():
            for mname, _, _ in MODES:
                m = e[mname]
                cells = [f"{m[k]['median']} ({m[k]['min']}-{m[k]['max']})" for k in ("skip", "noskip", "rowlinear")]
                print(f"| {cname} | {mname} | {cells[0]} | {cells[1]} | {cells[2]} | {m['bytes']:,} |")
            r = e["raycast_device"]
            print(f"| {cname} | `ocean_raycast_device`, same rays | {r['skip']['median']} ({r['skip']['min']}-{r['skip']['max']}) | "
                  f"{r['noskip']['median']} ({r['noskip']['min']}-{r['noskip']['max']}) | | {r['bytes_up_and_down']:,} up and down |")


if __name__ == "__main__":
    main()
