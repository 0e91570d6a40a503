"""The hosts' velocity: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "velocity" mode -- a
context with OCEAN_F_VELOCITY, F steps, then one WaterBody::Velocity of water_body.h for five points -- against
the Python binding for the same seed and frames, bit for bit; and the Python facade's
WaterBody.GetWaterVelocity against OceanContext.query_velocity."""
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


def test_cpp_host_velocity(tmp_path):
    n, C, F, M = 256, 3, 3, 5
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "velocity"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["points"], summary["n"], summary["cascades"]) == (F, M, n, C)
    assert not os.path.exists(os.path.join(tmp_path, "buoyancy0.bin"))  # no slice was read back
    points = np.fromfile(os.path.join(tmp_path, "velocity_points.bin"), np.float32).reshape(M, 2)
    records = np.fromfile(os.path.join(tmp_path, "velocity.bin"), np.float32).reshape(M, 8)
    np.testing.assert_array_equal(np.float32(summary["records"]).reshape(M, 8), records)  # printed with %.9g: exact
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS | oh.F_VELOCITY)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    want = ctx.query_velocity(points)  # 4 steps: the facade's default
    ctx.close()
    np.testing.assert_array_equal(records, want)
    assert np.abs(records[:, :3]).max() > 0 and np.isfinite(records).all()


def test_water_body_get_water_velocity_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes", velocity=True).Awake()
    assert wb.ctx.flags & oh.F_VELOCITY
    wb.Update(0.5)
    for pos in ((0.0, 3.0, 0.0), (37.5, 0.0, -12.25), (-410.0, 1.0, 250.75)):
        got = wb.GetWaterVelocity(pos)
        assert got.shape == (3,) and got.dtype == np.float32
        np.testing.assert_array_equal(got, wb.ctx.query_velocity(np.float32([[pos[0], pos[2]]]))[0, :3])
        np.testing.assert_array_equal(wb.GetWaterVelocity(pos, iterations=0),
                                      wb.ctx.query_velocity(np.float32([[pos[0], pos[2]]]), iterations=0)[0, :3])
    wb.OnDisable()
    # without `velocity` the facade creates the context it always did, and the query says so
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    assert not wb.ctx.flags & oh.F_VELOCITY
    wb.Update(0.5)
    with pytest.raises(oh.OceanError) as e:
        wb.GetWaterVelocity((0.0, 0.0, 0.0))
    assert e.value.code == oh.E_UNSUPPORTED
    wb.OnDisable()
