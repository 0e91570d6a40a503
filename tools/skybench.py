#!/usr/bin/env python3
"""The atmosphere (csrc/atmosphere.hip) and the camera's sky mode (csrc/view.hip, k_camera_sky), kernel time by events
(ocean_set_kernel_timing, kind 2), in one run:

    python tools/skybench.py [--rounds 5] [--launches 10] [--markdown]

1. ocean_atmosphere at AtmosphereController's sizes (64 x 256, 64 x 64): the transmittance and the multiscatter launch
   together, then each alone by difference of a run that stops after the first (the two are one entry).
2. ocean_sky_update alone (256 x 128): the per-frame cost.
3. tools/camerabench.py's context (4 x 1024^2, K = 2, S = 64, B = 8) and its two cameras, a 1024 x 1024 colour image
   with OCEAN_CAMERA_COLOR and with OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT, alternating rounds on one context.
Each figure is the median over the rounds with its range.  Prints one JSON line; --markdown appends the table of
docs/MEASUREMENTS.md.  A record, not a gate."""
import argparse
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "ocean-simulation_amd"))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import torch  # noqa: E402,F401  (one HIP runtime per process: torch first)
import ocean_hip as oh  # noqa: E402
from camerabench import H, K, B, S, W, cameras, make_context, summarize, timed_kind2  # noqa: E402

vp = ctypes.c_void_p
SUN = (0.3, 0.5, 0.4)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--markdown", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "skybench needs a GPU"
    ctx = make_context({})
    res = {"dims": list(oh.ATMOSPHERE_DEFAULT_DIMS), "width": W, "height": H, "k": K, "steps": S, "refine": B}
    # the two launches of ocean_atmosphere, and the transmittance table alone: a 64 x 256 multiscatter table of 2 x 2
    # texels costs one workgroup beside it, which the difference removes again
    both = [timed_kind2(ctx, lambda: ctx.atmosphere(), a.launches, 2) for _ in range(a.rounds)]
    res["atmosphere_us"] = summarize(both)
    small = (64, 256, 2, 2, 256, 128)
    first = [timed_kind2(ctx, lambda: ctx.atmosphere(None, small), a.launches, 2) for _ in range(a.rounds)]
    res["transmittance_plus_2x2_multiscatter_us"] = summarize(first)
    ctx.atmosphere()
    res["sky_update_us"] = summarize([timed_kind2(ctx, lambda: ctx.sky_update(SUN), a.launches) for _ in range(a.rounds)])
    res["kernel"] = ctx.kernel_name(2)
    mat = oh.material(roughness=0.3, lod_slope=0.004, light_direction=SUN, light_color=ctx.sun_color(SUN))
    out = torch.empty(W * H * 4, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    res["cameras"] = {}
    for cname, cam in cameras():
        fns = {name: (lambda mode=mode: oh._check(ctx.lib.ocean_camera_device(
            ctx._h, 0, mode, K, S, B, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H, vp(out.data_ptr()), W * H * 16),
            "ocean_camera_device")) for name, mode in (("color", oh.CAMERA_COLOR), ("sky_lut", oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT))}
        times = {k: [] for k in fns}
        for _ in range(a.rounds):
            for k, fn in fns.items():
                times[k].append(timed_kind2(ctx, fn, a.launches))
        res["cameras"][cname] = {k: summarize(v) for k, v in times.items()}
    ctx.close()
    print(json.dumps(res))
    if a.markdown:
        print("\n| what | kernel time (us) |")
        print("|---|---|")
        for k in ("atmosphere_us", "transmittance_plus_2x2_multiscatter_us", "sky_update_us"):
            m = res[k]
            print(f"| {k} | {m['median']} ({m['min']}-{m['max']}) |")
        for cname, e in res["cameras"].items():
            for k, m in e.items():
                print(f"| camera {cname}, {k} | {m['median']} ({m['min']}-{m['max']}) |")


if __name__ == "__main__":
    main()
