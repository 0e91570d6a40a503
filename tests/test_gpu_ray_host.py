"""The hosts' ray casts and bounds: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "rays" mode --
F steps, then one WaterBody::Raycast of water_body.h for six rays and one WaterBody::SurfaceBounds -- against the
Python binding for the same seed and frames, bit for bit."""
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


def test_cpp_host_rays(tmp_path):
    n, C, F, M = 256, 3, 3, 6
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "rays"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["rays"], summary["n"], summary["cascades"]) == (F, M, n, C)
    assert not os.path.exists(os.path.join(tmp_path, "buoyancy0.bin"))  # no slice was read back
    rays = np.fromfile(os.path.join(tmp_path, "rays.bin"), np.float32).reshape(M, 8)
    records = np.fromfile(os.path.join(tmp_path, "raycast.bin"), np.float32).reshape(M, 8)
    bounds = np.fromfile(os.path.join(tmp_path, "bounds.bin"), np.float32).reshape(C, 8)
    np.testing.assert_array_equal(np.float32(summary["records"]).reshape(M, 8), records)  # printed with %.9g: exact
    np.testing.assert_array_equal(np.float32(summary["bounds"]).reshape(C, 8), bounds)
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    want = ctx.raycast(rays, iterations=4, steps=32, refine=8)
    want_bounds = ctx.surface_bounds()
    ctx.close()
    np.testing.assert_array_equal(records, want)
    np.testing.assert_array_equal(bounds, want_bounds)
    assert np.isfinite(records).all() and (bounds[:, 5] > 0).all() and (bounds[:, 1] < 0).all()
    # the six rays were chosen to meet every status: down and slanted rays hit, level and climbing ones miss, and
    # the one from 50 m down starts under water
    np.testing.assert_array_equal(records[:, 3], np.float32([oh.RAY_HIT, oh.RAY_HIT, oh.RAY_HIT, oh.RAY_MISS,
                                                             oh.RAY_MISS, oh.RAY_SUBMERGED]))
