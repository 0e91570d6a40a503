#!/usr/bin/env python3
"""The camera views that see the bodies (csrc/view.hip, k_camera_bodies) at cfg3's shape and parameters: one context
of 4 x 1024^2 with the scene's cascades, K = 2, S = 64, B = 8, a 1024 x 1024 image, from camerabench.py's horizon camera
and its straight-down camera.

    python tools/bodyviewbench.py [--rounds 3] [--launches 3] [--markdown]

1. The price of the new path with nothing to see: ocean_camera_device against ocean_camera_bodies_device with count = 0,
   in the three modes, same context, alternating rounds; the two images are compared bit for bit.
2. 64, 1024 and 8192 boxes in the view, RANGE mode, with the cull (the default) and with OCEAN_CAMERA_CULL=0, two
   contexts on the same frame; the images are compared bit for bit.  Two scenes per count: `few`, boxes of about a
   metre, which cover few pixels, and `most`, the same boxes grown until they cover most of the image, where the march
   stops at the body for most rays.  The share of body pixels is reported with each.
3. The host's alternative for 64 boxes: ocean_camera_device in HITS mode (kernel time), the copy of its 32 MiB to the
   host (wall time), and the box test of tests/test_camera_bodies_abi.py's restatement on the CPU (wall time, numpy).
Kernel times are by events (ocean_set_kernel_timing, kind 2), the median over the rounds with its range.  Prints one
JSON line; --markdown appends the tables of docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from camerabench import B, H, K, MODES, S, W, cameras, make_context, pixel_rays, summarize, timed_kind2  # noqa: E402

COUNTS = (64, 1024, 8192)
BOX = np.float32([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
PAINT = np.float32([0.85, 0.35, 0.15, 0.6])
vp = ctypes.c_void_p
f32 = np.float32


def boxes(cam, count, grow, seed=11):
    """`count` boxes float32[count][10] where pixels of the image look: each at a random pixel's ray, where that ray
    crosses the level y = 0.5 (the horizon camera: at most 1500 m away) or 15 m along it, of about one metre times
    `grow` times its distance over 20 m, any orientation."""
    rng = np.random.default_rng(seed)
    rays = pixel_rays(cam)[rng.integers(0, W * H, count)].astype(np.float64)
    o, d = rays[:, 0:3], rays[:, 3:6]
    with np.errstate(divide="ignore", invalid="ignore"):
        t = np.where(d[:, 1] < -1e-3, (0.5 - o[:, 1]) / d[:, 1], np.inf)
    t = np.where(t <= 1500.0, t, rng.uniform(15.0, 400.0, count))
    rec = np.empty((count, 10))
    rec[:, 0:3] = o + t[:, None] * d
    q = rng.normal(size=(count, 4))
    rec[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None]
    rec[:, 7:10] = rng.uniform(0.7, 1.4, (count, 3)) * (1.0 + (grow - 1.0) * t[:, None] / 20.0)
    return rec.astype(f32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bodyviewbench needs a GPU"
    ctxs = {"cull": make_context({"OCEAN_CAMERA_CULL": "1"}), "nocull": make_context({"OCEAN_CAMERA_CULL": "0"})}
    ctx = ctxs["cull"]
    dev = torch.device("cuda", ctx.device)
    mat = oh.material(roughness=0.3, lod_slope=0.004)
    out = {k: torch.empty(W * H * 8, dtype=torch.float32, device=dev) for k in ("a", "b")}

    def bodies_call(c, mode, per, cam, d_bodies, count, o):
        return lambda: oh._check(c.lib.ocean_camera_bodies_device(
            c._h, 0, mode, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(BOX.ctypes.data),
            vp(PAINT.ctypes.data), vp(d_bodies.data_ptr()) if count else None, 10, count, vp(o.data_ptr()),
            W * H * per * 4), "ocean_camera_bodies_device")

    res = {"n": 1024, "cascades": 4, "width": W, "height": H, "k": K, "steps": S, "refine": B, "cameras": {}}
    for cname, cam in cameras():
        entry = {"empty": {}, "counts": {}}
        # 1. nothing to see
        for mname, mode, per in MODES:
            plain = lambda: oh._check(ctx.lib.ocean_camera_device(  # noqa: E731
                ctx._h, 0, mode, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(out["a"].data_ptr()),
                W * H * per * 4), "ocean_camera_device")
            empty = bodies_call(ctx, mode, per, cam, None, 0, out["b"])
            times = {"camera": [], "bodies_count_0": []}
            for _ in range(a.rounds):
                times["camera"].append(timed_kind2(ctx, plain, a.launches))
                times["bodies_count_0"].append(timed_kind2(ctx, empty, a.launches))
            torch.cuda.synchronize()
            n = W * H * per
            assert torch.equal(out["a"][:n].view(torch.int32), out["b"][:n].view(torch.int32))
            entry["empty"][mname] = {k: summarize(v) for k, v in times.items()}
        # 2. the counts, with and without the cull
        for count in COUNTS:
            for scene, grow in (("few", 1.0), ("most", 12.0 * (64.0 / count) ** 0.5 + 1.0)):
                rec = boxes(cam, count, grow)
                d_bodies = torch.from_numpy(rec).to(dev)
                torch.cuda.synchronize()
                fns = {"cull": bodies_call(ctxs["cull"], oh.CAMERA_RANGE, 1, cam, d_bodies, count, out["a"]),
                       "nocull": bodies_call(ctxs["nocull"], oh.CAMERA_RANGE, 1, cam, d_bodies, count, out["b"])}
                times = {k: [] for k in fns}
                for _ in range(a.rounds):
                    for k in fns:
                        times[k].append(timed_kind2(ctxs[k], fns[k], a.launches if k == "cull" or count < 8192 else 1))
                torch.cuda.synchronize()
                assert torch.equal(out["a"][:W * H].view(torch.int32), out["b"][:W * H].view(torch.int32))
                hits = torch.empty(W * H * 8, dtype=torch.float32, device=dev)
                bodies_call(ctx, oh.CAMERA_HITS, 8, cam, d_bodies, count, hits)()
                ctx.synchronize()
                share = float((hits.view(-1, 8)[:, 3] == oh.RAY_BODY).float().mean())
                entry["counts"][f"{count}_{scene}"] = {"body_share": round(share, 3),
                                                       **{k: summarize(v) for k, v in times.items()}}
        # 3. the host's alternative for 64 boxes
        from test_camera_bodies_abi import body_pixels, compose
        plain = lambda: oh._check(ctx.lib.ocean_camera_device(  # noqa: E731
            ctx._h, 0, oh.CAMERA_HITS, K, S, B, vp(cam.ctypes.data), None, W, H, vp(out["a"].data_ptr()), W * H * 32),
            "ocean_camera_device")
        kernel_us = summarize([timed_kind2(ctx, plain, a.launches) for _ in range(a.rounds)])
        torch.cuda.synchronize()
        t = time.perf_counter()
        landed = out["a"].cpu().numpy().reshape(-1, 8)
        copy_ms = 1e3 * (time.perf_counter() - t)
        t = time.perf_counter()
        b, te, _ = body_pixels(pixel_rays(cam), BOX, boxes(cam, 64, 1.0))
        compose(landed, b, te)
        cpu_ms = 1e3 * (time.perf_counter() - t)
        entry["host_alternative_64"] = {"hits_kernel_us": kernel_us, "copy_32MiB_wall_ms": round(copy_ms, 1),
                                        "cpu_box_test_numpy_wall_ms": round(cpu_ms, 1)}
        res["cameras"][cname] = entry
    for c in ctxs.values():
        c.close()
    print(json.dumps(res))
    if a.markdown:
        cell = lambda m: f"{m['median']} ({m['min']}-{m['max']})"  # noqa: E731
        print("\n| camera | mode | `ocean_camera_device` (us) | `ocean_camera_bodies_device`, count = 0 (us) |")
        print("|---|---|---|---|")
        for cname, e in res["cameras"].items():
            for mname, m in e["empty"].items():
                print(f"| {cname} | {mname} | {cell(m['camera'])} | {cell(m['bodies_count_0'])} |")
        print("\n| camera | boxes, scene | body pixels | cull (us) | OCEAN_CAMERA_CULL=0 (us) |")
        print("|---|---|---|---|---|")
        for cname, e in res["cameras"].items():
            for key, m in e["counts"].items():
                print(f"| {cname} | {key.replace('_', ', ')} | {m['body_share']} | {cell(m['cull'])} | {cell(m['nocull'])} |")
        for cname, e in res["cameras"].items():
            h = e["host_alternative_64"]
            print(f"\n{cname}: the host's alternative for 64 boxes: HITS kernel {cell(h['hits_kernel_us'])} us, copy of 32 MiB "
                  f"{h['copy_32MiB_wall_ms']} ms (wall), CPU box test {h['cpu_box_test_numpy_wall_ms']} ms (numpy, wall)")


if __name__ == "__main__":
    main()
