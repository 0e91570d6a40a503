"""The hosts' Dynamics: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "dynamics" mode -- a
velocity context, F steps, then one WaterBody::Dynamics of water_body.h for the buoyancy mode's five boxes of 12
probes with five fixed motions -- against the Python binding for the same seed and frames, bit for bit (both
hosts drive the same library with the same inputs, as tests/test_gpu_body_host.py has it); and the Python
facade's WaterBody.Dynamics against OceanContext.body_dynamics."""
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


def test_cpp_host_dynamics(tmp_path):
    n, C, F, M, P = 64, 3, 3, 5, 12
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "dynamics"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["probes"], summary["bodies"]) == (F, P, M)
    assert not os.path.exists(os.path.join(tmp_path, "buoyancy.bin"))  # the buoyancy mode's file is not this mode's
    hull = np.fromfile(os.path.join(tmp_path, "hull.bin"), np.float32).reshape(P, 5)
    bodies = np.fromfile(os.path.join(tmp_path, "bodies.bin"), np.float32).reshape(M, 10)
    motion = np.fromfile(os.path.join(tmp_path, "motion.bin"), np.float32).reshape(M, 6)
    records = np.fromfile(os.path.join(tmp_path, "dynamics.bin"), np.float32).reshape(M, 16)
    np.testing.assert_array_equal(np.float32(summary["records"]).reshape(M, 16), records)  # printed with %.9g: exact
    np.testing.assert_allclose(hull, oh.OceanContext.box_hull(4, 3), rtol=0, atol=1e-7)
    assert not motion[0].any() and motion[1:].any(axis=1).all()
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS | oh.F_VELOCITY)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    want = ctx.body_dynamics(hull, bodies, motion)  # surface mode, 4 steps, linear drag: the facade's defaults
    np.testing.assert_array_equal(want[:, :8], ctx.body_buoyancy(hull, bodies))
    ctx.close()
    np.testing.assert_array_equal(records, want)
    assert (records[:, 0] > 0).any() and np.isfinite(records).all()
    assert np.abs(records[:, 8:14]).max() > 0 and (records[:, 15] > 0).any()


def test_water_body_dynamics_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes", velocity=True).Awake()
    wb.Update(0.5)
    hull = oh.OceanContext.box_hull(3, 2, ny=2)
    rng = np.random.default_rng(8)
    bodies = np.zeros((20, 10), np.float32)
    bodies[:, :3] = rng.uniform(-50.0, 50.0, (20, 3)) * [1.0, 0.02, 1.0]
    q = rng.standard_normal((20, 4))
    bodies[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    bodies[:, 7:10] = rng.uniform(0.5, 3.0, (20, 3))
    motion = rng.uniform(-1.0, 1.0, (20, 6)).astype(np.float32)
    got = wb.Dynamics(hull, bodies, motion)
    assert got.shape == (20, 16) and (got[:, 15] > 0).any()
    np.testing.assert_array_equal(got, wb.ctx.body_dynamics(hull, bodies, motion))
    np.testing.assert_array_equal(wb.Dynamics(hull, bodies, motion, iterations=0, mode=oh.QUERY_REFERENCE,
                                              law=oh.DRAG_QUADRATIC),
                                  wb.ctx.body_dynamics(hull, bodies, motion, 0, oh.QUERY_REFERENCE, oh.DRAG_QUADRATIC))
    wb.OnDisable()
