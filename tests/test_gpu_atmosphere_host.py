"""The hosts' atmosphere: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "sky" mode -- the
atmosphere's tables at the sizes 12 x 20, 3 x 5 and 20 x 12, F steps, one WaterBody::SkyUpdate of water_body.h and the
camera's OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT picture under the light colour it returned -- against the Python
binding for the same seed and frames, bit for bit."""
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


def test_cpp_host_sky(tmp_path):
    n, C, F, w, h = 128, 2, 2, 32, 24
    dims = (12, 20, 3, 5, 20, 12)
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "sky"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["n"], summary["cascades"], summary["width"], summary["height"]) == (F, n, C, w, h)
    assert tuple(summary["dims"]) == dims

    def load(name):
        return np.fromfile(os.path.join(tmp_path, name), np.float32)

    cam, mat, sun = load("camera.bin"), load("material.bin"), load("sun.bin")
    assert cam.shape == (oh.CAMERA_FLOATS,) and mat.shape == (oh.CAMERA_MATERIAL_FLOATS,) and sun.shape == (3,)
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    ctx.atmosphere(None, dims)
    for f in range(F):
        ctx.step(f / 60.0)
    ctx.sky_update(sun)
    rgb = ctx.sun_color(sun)
    np.testing.assert_array_equal(load("sun_color.bin"), rgb)
    np.testing.assert_array_equal(mat[23:26], rgb)
    np.testing.assert_allclose(np.linalg.norm(mat[20:23].astype(np.float64)), 1.0, atol=1e-6)
    for k, name in enumerate(("transmittance.bin", "multiscatter.bin", "skyview.bin")):
        want = ctx.atmosphere_lut(k)
        assert want.shape == (dims[2 * k + 1], dims[2 * k], 4)
        np.testing.assert_array_equal(load(name).reshape(want.shape), want, err_msg=name)
    color = load("sky_color.bin").reshape(h, w, 4)
    want = ctx.camera(cam, w, h, oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT, mat, 0, 2, 32, 6)
    ctx.close()
    np.testing.assert_array_equal(color, want)
    status = color[..., 3]
    assert (summary["miss"], summary["hit"], summary["submerged"]) == \
        ((status == oh.RAY_MISS).sum(), (status == oh.RAY_HIT).sum(), 0)
    # the horizon crosses the image, and the sky is not the two-colour one (material[26..31] are zero)
    assert summary["hit"] >= w * h // 5 and summary["miss"] >= w * h // 5
    assert np.isfinite(color).all() and (color[status == oh.RAY_MISS, :3] > 0).all()
