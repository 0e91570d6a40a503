#!/usr/bin/env python3
"""The camera views in which the water sees the bodies (csrc/view.hip, k_camera_scene) at cfg3's shape and parameters:
one context of 4 x 1024^2 with the scene's cascades, K = 2, S = 64, B = 8, a 1024 x 1024 image, from camerabench.py's
horizon camera and its straight-down camera, COLOR mode, under a low sun.

    python tools/scenebench.py [--rounds 3] [--launches 3] [--markdown]

Per camera and per count of bodyviewbench.py's metre-sized boxes (0, 64, 1024, 8192), in one run on the same frame:
ocean_camera_bodies_device; ocean_camera_scene_device at reach 10 m and 100 m with the culls (the default); the same
with OCEAN_CAMERA_CULL=0 on a second context.  The images with and without the culls are compared bit for bit, and the
shares of shadowed, through-water and mirrored water pixels come from one LINKS image per case.
Kernel times are by events (ocean_set_kernel_timing, kind 2), the median over the rounds with its range.  Prints one
JSON line; --markdown appends the table of docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from bodyviewbench import BOX, PAINT, boxes  # noqa: E402
from camerabench import B, H, K, S, W, cameras, make_context, summarize, timed_kind2  # noqa: E402

COUNTS = (0, 64, 1024, 8192)
REACHES = (10.0, 100.0)
SUN = (-0.55, 0.33, 0.35)
vp = ctypes.c_void_p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "scenebench needs a GPU"
    ctxs = {"cull": make_context({"OCEAN_CAMERA_CULL": "1"}), "nocull": make_context({"OCEAN_CAMERA_CULL": "0"})}
    ctx = ctxs["cull"]
    dev = torch.device("cuda", ctx.device)
    mat = oh.material(roughness=0.3, lod_slope=0.004, light_direction=SUN)
    out = {k: torch.empty(W * H * 4, dtype=torch.float32, device=dev) for k in ("a", "b")}

    def ptr(d_bodies, count):
        return vp(d_bodies.data_ptr()) if count else None

    def bodies_call(c, cam, d_bodies, count, o):
        return lambda: oh._check(c.lib.ocean_camera_bodies_device(
            c._h, 0, oh.CAMERA_COLOR, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(BOX.ctypes.data),
            vp(PAINT.ctypes.data), ptr(d_bodies, count), 10, count, vp(o.data_ptr()), W * H * 16),
            "ocean_camera_bodies_device")

    def scene_call(c, mode, cam, op, d_bodies, count, o):
        return lambda: oh._check(c.lib.ocean_camera_scene_device(
            c._h, 0, mode, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(BOX.ctypes.data),
            vp(PAINT.ctypes.data), vp(op.ctypes.data), ptr(d_bodies, count), 10, count, vp(o.data_ptr()), W * H * 16),
            "ocean_camera_scene_device")

    res = {"n": 1024, "cascades": 4, "width": W, "height": H, "k": K, "steps": S, "refine": B, "cameras": {}}
    for cname, cam in cameras():
        entry = {}
        for count in COUNTS:
            rec = boxes(cam, max(count, 1), 1.0)
            d_bodies = torch.from_numpy(rec).to(dev)
            torch.cuda.synchronize()
            row = {"bodies": summarize([timed_kind2(ctx, bodies_call(ctx, cam, d_bodies, count, out["a"]), a.launches)
                                        for _ in range(a.rounds)])}
            for reach in REACHES:
                op = oh.optics(shadow_color=(0.02, 0.03, 0.08), shadow_intensity=0.6, fog_density=0.15, reach=reach)
                fns = {"cull": scene_call(ctxs["cull"], oh.CAMERA_COLOR, cam, op, d_bodies, count, out["a"]),
                       "nocull": scene_call(ctxs["nocull"], oh.CAMERA_COLOR, cam, op, d_bodies, count, out["b"])}
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k in fns:
                        times[k].append(timed_kind2(ctxs[k], fns[k], a.launches if k == "cull" or count < 8192 else 1))
                torch.cuda.synchronize()
                assert torch.equal(out["a"].view(torch.int32), out["b"].view(torch.int32))
                scene_call(ctx, oh.CAMERA_LINKS, cam, op, d_bodies, count, out["a"])()
                ctx.synchronize()
                links = out["a"].view(-1, 4)
                water = links[:, 3] == oh.RAY_HIT
                share = lambda m: round(float((m & water).float().sum() / max(int(water.sum()), 1)), 4)  # noqa: E731
                row[f"reach_{int(reach)}"] = {"shadowed": share(links[:, 0] == 0), "through": share(links[:, 1] >= 0),
                                              "mirrored": share(links[:, 2] >= 0),
                                              **{k: summarize(v) for k, v in times.items()}}
            entry[str(count)] = row
        res["cameras"][cname] = entry
    for c in ctxs.values():
        c.close()
    print(json.dumps(res))
    if a.markdown:
        cell = lambda m: f"{m['median']} ({m['min']}-{m['max']})"  # noqa: E731
        print("\n| camera | boxes | `ocean_camera_bodies_device` (us) | reach (m) | shadowed / through / mirrored water pixels "
              "| `ocean_camera_scene_device` (us) | OCEAN_CAMERA_CULL=0 (us) |")
        print("|---|---|---|---|---|---|---|")
        for cname, e in res["cameras"].items():
            for count, row in e.items():
                for reach in REACHES:
                    m = row[f"reach_{int(reach)}"]
                    print(f"| {cname} | {count} | {cell(row['bodies'])} | {int(reach)} | {m['shadowed']} / {m['through']} / "
                          f"{m['mirrored']} | {cell(m['cull'])} | {cell(m['nocull'])} |")


if __name__ == "__main__":
    main()
