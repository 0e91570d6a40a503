"""The hosts' spray particles: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "spray" mode -- F steps
on a velocity context, one WaterBody::Whitecaps over a 101 x 101 grid, then two WaterBody::Spray calls of water_body.h,
one that spawns from the list into an empty pool and one that advances that pool -- against the Python binding for
the same seed and frames, bit for bit."""
import json
import os
import subprocess

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

HOST = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ocean-simulation_amd", "host",
                    "abi_host")


def test_cpp_host_spray(tmp_path):
    n, C, F = 64, 4, 3  # (the scene's fourth cascade, 34 m, is the one that breaks at 64^2)
    grid, threshold, capacity, pool_capacity = (-500.0, -500.0, 10.0, 10.0, 101, 101), 0.1, 4096, 8192
    spray = oh.OceanContext.spray_params(1.0 / 240.0, 9.81, 0.5, (3.0, 0.0, 1.0), 2.0, 1.0, 8.0)
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "spray"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["n"], summary["cascades"], summary["capacity"]) == (F, n, C, pool_capacity)
    load = lambda name, rows: np.fromfile(os.path.join(tmp_path, name), np.float32).reshape(rows, 8)  # noqa: E731
    lst = load("spray_emitters.bin", capacity + 1)
    got = [load("spray0.bin", pool_capacity + 1), load("spray1.bin", pool_capacity + 1)]
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS | oh.F_VELOCITY)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    total, records = ctx.whitecaps(threshold, *grid, capacity=capacity)
    want_list = np.zeros((capacity + 1, 8), np.float32)
    want_list[0].view(np.uint32)[:4] = (total, len(records), 101 * 101, capacity)
    want_list[1:1 + len(records)] = records
    np.testing.assert_array_equal(lst.view(np.uint32), want_list.view(np.uint32))
    first = ctx.spray_step(spray, np.zeros((pool_capacity + 1, 8), np.float32), want_list, 4, 2)
    second = ctx.spray_step(spray, first, None, 4, 2)
    ctx.close()
    for k, (g, w) in enumerate(zip(got, (first, second))):
        t, m, rec = oh.OceanContext.parse_spray(g)
        wt, wm, wrec = oh.OceanContext.parse_spray(w)
        assert (t, m) == (wt, wm) == (summary["survivors"][k], summary["candidates"][k])
        assert summary["written"][k] == len(rec) == len(wrec)
        np.testing.assert_array_equal(rec.view(np.uint32), wrec.view(np.uint32))
        assert not g[1 + len(rec):].any()  # the host clears what the library leaves unspecified
    # the list spawned particles, and some of them fly
    e = len(records)
    assert summary["candidates"] == [e, summary["written"][0]]
    assert 0 < summary["survivors"][1] <= summary["survivors"][0] <= e
