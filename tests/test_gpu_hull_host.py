"""The hosts' Hydrostatics: the compiled C++ host (ocean-simulation_amd/host/abi_host) in its "hydrostatics" mode -- F
steps, then one WaterBody::Hydrostatics of water_body.h for five boxes of the 12-triangle mesh -- against the Python
binding for the same seed and frames, bit for bit; the Python facade's WaterBody.Hydrostatics against
OceanContext.body_hydrostatics; and one play of the sequence host (abi_sequence) that interleaves steps and the call."""
import json
import os

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_host_sequences import make_ctx, run_once

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
HOST_DIR = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "ocean-simulation_amd", "host")
HOST, SEQUENCE = os.path.join(HOST_DIR, "abi_host"), os.path.join(HOST_DIR, "abi_sequence")
BODIES = f32([[0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0, 1.0, 1.0, 1.0], [37.5, 0.25, -12.25, 0.5, 0.5, 0.5, 0.5, 1.5, 2.0, 0.5],
              [-410.0, -0.5, 250.75, 0.0, 0.0, 0.6, 0.8, 2.0, 1.5, 1.0]])


def test_cpp_host_hydrostatics(tmp_path):
    n, C, F, M, V, T = 256, 3, 3, 5, 8, 12
    assert os.path.exists(HOST), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    r = run_once([HOST, str(tmp_path), str(n), str(C), str(F), "hydrostatics"])
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert (summary["frames"], summary["vertices"], summary["triangles"], summary["bodies"]) == (F, V, T, M)
    assert not os.path.exists(os.path.join(tmp_path, "buoyancy0.bin"))  # no slice was read back
    verts = np.fromfile(os.path.join(tmp_path, "vertices.bin"), f32).reshape(V, 3)
    tris = np.fromfile(os.path.join(tmp_path, "triangles.bin"), np.int32).reshape(T, 3)
    bodies = np.fromfile(os.path.join(tmp_path, "bodies.bin"), f32).reshape(M, 10)
    records = np.fromfile(os.path.join(tmp_path, "hydrostatics.bin"), f32).reshape(M, 16)
    np.testing.assert_array_equal(f32(summary["records"]).reshape(M, 16), records)  # printed with %.9g: exact
    # the host's mesh is the box 2 x 1 x 3, closed and wound outward, as box_mesh(2, 1, 3) is
    want_v, want_t = oh.OceanContext.box_mesh(2, 1, 3)
    assert sorted(map(tuple, verts)) == sorted(map(tuple, want_v)) and tris.min() == 0 and tris.max() == V - 1
    p = verts.astype(np.float64)[tris]
    av = 0.5 * np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    assert np.abs(av.sum(axis=0)).max() == 0 and (np.einsum("ij,ij->i", av, p.mean(axis=1)) > 0).all()
    assert np.einsum("ij,ij->i", av, p[:, 0]).sum() / 3 == 6.0 and want_t.shape == tris.shape
    ctx = oh.OceanContext(n, C, 1, oh.F_MIPS)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:C])
    ctx.generate_noise(42)
    ctx.init_spectrum()
    for f in range(F):
        ctx.step(f / 60.0)
    want = ctx.body_hydrostatics(verts, tris, bodies)  # 4 steps: the facade's default
    ctx.close()
    np.testing.assert_array_equal(records, want)
    assert (records[:, 1] > 0).any() and (records[:, 3] > 0).any() and np.isfinite(records).all()


def test_water_body_hydrostatics_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    wb.Update(0.5)
    verts, tris = oh.OceanContext.box_mesh(2, 1, 3, 2, 1, 3)
    rng = np.random.default_rng(8)
    bodies = np.zeros((20, 10), f32)
    bodies[:, :3] = rng.uniform(-50.0, 50.0, (20, 3)) * [1.0, 0.02, 1.0]
    q = rng.standard_normal((20, 4))
    bodies[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    bodies[:, 7:10] = rng.uniform(0.5, 3.0, (20, 3))
    got = wb.Hydrostatics(verts, tris, bodies)
    assert got.shape == (20, 16) and (got[:, 1] > 0).any()
    np.testing.assert_array_equal(got, wb.ctx.body_hydrostatics(verts, tris, bodies))
    np.testing.assert_array_equal(wb.Hydrostatics(verts, tris, bodies, iterations=0),
                                  wb.ctx.body_hydrostatics(verts, tris, bodies, 0))
    wb.OnDisable()


def test_sequence_host_plays_hydrostatics_between_steps(tmp_path):
    """step, X, step, X (another mesh and K, more bodies), X again, a surface query between, X of the first shape: every
    result of the one process equals the binding's for the same sequence, bit for bit."""
    n, C, flags = 64, 2, oh.F_MIPS
    assert os.path.exists(SEQUENCE), "build it: make -C ocean-simulation_amd (or __graft_entry__.build())"
    small, big = oh.OceanContext.box_mesh(2, 1, 3), oh.OceanContext.box_mesh(2, 1, 3, 8, 8, 4)
    more = np.concatenate([BODIES, BODIES + f32([3, 0.1, -2, 0, 0, 0, 0, 0, 0, 0])])
    points = np.ascontiguousarray(BODIES[:, [0, 2]])
    plays = [("step", 0.25), ("hull", 4, small, BODIES), ("step", 0.5), ("hull", 2, big, more), ("hull", 2, big, more),
             ("query", points), ("hull", 4, small, BODIES)]
    lines = []
    for k, p in enumerate(plays):
        if p[0] == "step":
            lines.append(f"step {p[1]!r}")
        elif p[0] == "query":
            p[1].tofile(os.path.join(tmp_path, f"in_{k}_p.bin"))
            lines.append(f"query_surface {oh.QUERY_SURFACE} 4 in_{k}_p.bin")
        else:
            _, iterations, (verts, tris), bodies = p
            verts.tofile(os.path.join(tmp_path, f"in_{k}_v.bin"))
            tris.astype(np.int32).tofile(os.path.join(tmp_path, f"in_{k}_t.bin"))
            bodies.tofile(os.path.join(tmp_path, f"in_{k}_b.bin"))
            lines.append(f"body_hydrostatics {iterations} in_{k}_v.bin in_{k}_t.bin in_{k}_b.bin")
    with open(os.path.join(tmp_path, "ops.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    r = run_once([SEQUENCE, str(tmp_path), str(n), str(C), str(flags)])
    summary = json.loads(r.stdout.strip().splitlines()[-1])
    assert [e["rc"] for e in summary["ops"]] == [oh.OK] * len(plays)
    ctx = make_ctx(n, C, flags, 42)
    for k, (p, e) in enumerate(zip(plays, summary["ops"])):
        if p[0] == "step":
            ctx.step(p[1])
            continue
        want = ctx.query_surface(p[1], 0, oh.QUERY_SURFACE, 4) if p[0] == "query" else \
            ctx.body_hydrostatics(*p[2], p[3], iterations=p[1])
        got = np.fromfile(os.path.join(tmp_path, f"out_{k}.bin"), f32)
        assert e["words"] == want.size == got.size and e["sentinel"] == 0, (k, e)
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=f"op {k} {e['op']}")
        assert np.isfinite(want).all() and want.any()
    ctx.close()
    assert summary["ops"][1]["words"] == 3 * 16 and summary["ops"][3]["words"] == 6 * 16
