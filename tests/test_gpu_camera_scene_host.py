"""The hosts' camera views in which the water sees the bodies: the compiled C++ host (ocean-simulation_amd/host/abi_host)
in its "camera_scene" mode -- F steps, then two WaterBody::CameraScene calls of water_body.h for a fixed camera, five
boxes, a low sun and fixed optics, the LINKS image and the colour image -- against the Python binding for the same seed
and frames, bit for bit."""
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


def test_cpp_host_camera_scene(tmp_path):
    n, C, F, w, h = 256, 3, 3, 45, 37
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = subprocess.run([HOST, str(tmp_path), str(n), str(C), str(F), "camera_scene"], capture_output=True, text=True,
                       timeout=120, env=dict(os.environ))
    assert r.returncode == 0, r.stderr
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["n"], summary["cascades"], summary["width"], summary["height"]) == (F, n, C, w, h)
    read = lambda name: np.fromfile(os.path.join(tmp_path, name + ".bin"), np.float32)  # noqa: E731
    cam, mat, box, paint, optics, flat = (read(k) for k in ("camera", "material", "box", "paint", "optics", "bodies"))
    assert cam.shape == (oh.CAMERA_FLOATS,) and mat.shape == (oh.CAMERA_MATERIAL_FLOATS,) and box.shape == (6,)
    assert paint.shape == (4,) and optics.shape == (oh.SCENE_OPTICS_FLOATS,) and flat.shape == (4 * 16 + 10,)
    links, color = read("scene_links").reshape(h, w, 4), read("scene_color").reshape(h, w, 4)
    bodies = np.stack([flat[16 * b:16 * b + 10] for b in range(5)])  # the first ten floats of each record
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    want_links = ctx.camera_scene(cam, w, h, bodies, box, None, optics, oh.CAMERA_LINKS, mat, 0, 2, 32, 6)
    want_color = ctx.camera_scene(cam, w, h, bodies, box, paint, optics, oh.CAMERA_COLOR, mat, 0, 2, 32, 6)
    plain = ctx.camera_bodies(cam, w, h, bodies, box, paint, oh.CAMERA_COLOR, mat, 0, 2, 32, 6)
    ctx.close()
    np.testing.assert_array_equal(links, want_links)
    np.testing.assert_array_equal(color, want_color)
    np.testing.assert_array_equal(color[..., 3], links[..., 3])
    water = links[..., 3] == oh.RAY_HIT
    got = (int(water.sum()), int((links[water, 0] == 0).sum()), int((links[water, 1] >= 0).sum()),
           int((links[water, 2] >= 0).sum()))
    assert (summary["water"], summary["shadowed"], summary["through"], summary["mirrored"]) == got
    free = (links[..., 0] == 1) & (links[..., 1] == -1) & (links[..., 2] == -1)
    np.testing.assert_array_equal(color[free | ~water], plain[free | ~water])
    assert np.isfinite(color).all() and got[0] >= w * h // 5
    print(dict(zip(("water", "shadowed", "through", "mirrored"), got)))
    assert (color[water & ~free] != plain[water & ~free]).any()
