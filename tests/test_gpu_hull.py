"""GPU tests of the mesh hulls (ocean_body_hydrostatics / _device / _async, csrc/hull.hip).  The entry is restated in
numpy fp32 by restate_hull of tests/test_hull_math.py -- the transform, the clip and the per-piece terms as
include/ocean/ocean.h orders them, the surface lookup by restate_surface of tests/test_gpu_query.py over the context's own
read-back textures, the sums by the 256-lane tree -- and the comparison is bit for bit."""
import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_body import max_height, random_quaternions
from test_gpu_query import Textures, make_ctx, restate_surface
from test_hull_math import flat, restate_hull

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
M = 5
# where the five bodies sit, in hull sizes above the sea's mean level: one deep, three across the surface, one high
LEVELS = (-1.5, -0.2, 0.0, 0.2, 1.5)


def soup(rng, nverts, ntris, size):
    """A triangle soup: vertices scattered over a cube of side `size`, triangles of three distinct random vertices."""
    verts = (rng.uniform(-0.5, 0.5, (nverts, 3)) * size).astype(f32)
    tris = np.stack([rng.permutation(nverts)[:3] for _ in range(ntris)]).astype(np.int32)
    return verts, tris


def hulls(rng, size):
    """(name, vertices, triangles): a lone triangle, the 8-vertex box, a box of 258 vertices and 512 triangles (two trips
    of both loops, the second of the vertices' a partial one), soups around one trip of the triangles (255, 256, 257) over
    two of the vertices, and the caps (2048, 4096: eight and sixteen trips)."""
    box = oh.OceanContext.box_mesh
    yield "triangle", (rng.uniform(-0.5, 0.5, (3, 3)) * size).astype(f32), np.int32([[0, 1, 2]])
    yield "box 8", *box(size, 0.5 * size, 0.75 * size)
    yield "box 258", *box(size, 0.5 * size, 0.75 * size, 8, 8, 4)
    for nverts, ntris in ((300, 255), (300, 256), (300, 257), (oh.HULL_MAX_VERTICES, oh.HULL_MAX_TRIANGLES)):
        yield f"soup {nverts} x {ntris}", *soup(rng, nverts, ntris, size)


def poses(rng, size, height):
    """Five bodies spread over +- 1.5 hull sizes about the sea's height range (+- height), anywhere on the sea, at any
    attitude, scaled by 0.8 .. 1.25 per axis."""
    b = np.empty((M, 10), f32)
    b[:, 0], b[:, 2] = rng.uniform(-2000.0, 2000.0, M), rng.uniform(-2000.0, 2000.0, M)
    b[:, 1] = np.float64(LEVELS) * size + rng.uniform(-1.0, 1.0, M) * height
    b[:, 3:7] = random_quaternions(rng, M)
    b[:, 7:10] = rng.uniform(0.8, 1.25, (M, 3))
    return b


def surface_lookup(tex, k):
    return lambda q: restate_surface(tex, q, (k,))[k]


CONTEXTS = [(64, 1, 0, 1, 0), (64, 4, 0, 1, 0), (128, 2, oh.F_MIPS, 1, 0), (128, 2, oh.F_DISPLACEMENT_ONLY, 1, 0),
            (64, 2, 0, 2, 1)]


@pytest.mark.parametrize("n,ncasc,flags,tiles,tile", CONTEXTS)
def test_hull_matches_restatement(n, ncasc, flags, tiles, tile):
    """Bit for bit against the restatement, K in {0, 4}, M = 5, every hull of hulls().  Over the context's triangles the
    restatement's own classification shows at least 10 % each of m = 0, 1, 2 and 3, so neither clip nor the dry and the
    full case can hide."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags, tiles=tiles)
    tex = Textures(ctx, cas, tile)
    height = max_height(tex.disp)
    assert height > 0.0
    size = 4.0 * height
    rng = np.random.default_rng(7000 * n + 10 * ncasc + tile)
    classes = {0: [], 4: []}
    for name, verts, tris in hulls(rng, size):
        bodies = poses(rng, size, height)
        for k in (0, 4):
            want, m = restate_hull(verts, tris, bodies, surface_lookup(tex, k))
            got = ctx.body_hydrostatics(verts, tris, bodies, iterations=k, tile=tile)
            assert got.shape == (M, 16) and np.isfinite(got).all()
            np.testing.assert_array_equal(got, want, err_msg=f"{name}, K = {k}")
            classes[k].append(m.ravel())
    for k, ms in classes.items():
        share = np.bincount(np.concatenate(ms), minlength=4) / sum(len(x) for x in ms)
        print(f"K = {k}: {sum(len(x) for x in ms)} triangles, m = 0, 1, 2, 3: " + ", ".join(f"{s:.3f}" for s in share))
        assert (share >= 0.10).all(), share
    # the default arguments: 4 steps, tile 0; the facade forwards
    if tile == 0:
        np.testing.assert_array_equal(ctx.body_hydrostatics(verts, tris, bodies), got)
    if flags & oh.F_DISPLACEMENT_ONLY:
        assert (got[:, 7] >= 0).all()
    ctx.close()


def test_hull_three_forms_agree_and_device_indices_are_clamped():
    """The blocking, the async and the device form give the same bits.  The device form cannot see the indices: with
    indices far outside [0, V) it reads no vertex but its own (the record is that of the clamped indices, which the
    restatement clamps alike) and stays finite."""
    import torch
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas)
    tex = Textures(ctx, cas)
    height = max_height(tex.disp)
    size = 4.0 * height
    rng = np.random.default_rng(31)
    verts, tris = soup(rng, 300, 257, size)
    bodies = poses(rng, size, height)
    want = ctx.body_hydrostatics(verts, tris, bodies)
    rb = ctx.body_hydrostatics_async(verts.copy(), tris.copy(), bodies.copy())
    np.testing.assert_array_equal(rb.data, want)
    slot = oh.PinnedBuffer(M * 64)
    np.testing.assert_array_equal(ctx.body_hydrostatics_async(verts, tris, bodies, buf=slot, iterations=0).data,
                                  ctx.body_hydrostatics(verts, tris, bodies, iterations=0))
    dev = torch.device("cuda", ctx.device)
    # the vertex array sits between two guards of NaN: a read outside it would poison the record
    guard = 4096
    dv = torch.full((guard + 300 * 3 + guard,), float("nan"), dtype=torch.float32, device=dev)
    dv[guard:guard + 900] = torch.from_numpy(verts.ravel()).to(dev)
    dt = torch.from_numpy(tris.ravel()).to(dev)
    db = torch.from_numpy(bodies.ravel()).to(dev)
    o = torch.zeros(M * 16, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    vptr = dv.data_ptr() + guard * 4
    ctx.body_hydrostatics_device(vptr, 300, dt.data_ptr(), 257, db.data_ptr(), M, o.data_ptr())
    ctx.synchronize()
    np.testing.assert_array_equal(o.cpu().numpy().reshape(M, 16), want)
    wild = tris.copy()
    wild[::3, 0], wild[1::3, 1], wild[2::3, 2] = -1, 300, 1 << 30
    wild[5] = (-(1 << 31), (1 << 31) - 1, -7)
    dw = torch.from_numpy(wild.ravel()).to(dev)
    torch.cuda.synchronize()
    ctx.body_hydrostatics_device(vptr, 300, dw.data_ptr(), 257, db.data_ptr(), M, o.data_ptr())
    ctx.body_hydrostatics_device(vptr, 300, dw.data_ptr(), 257, db.data_ptr(), 0, o.data_ptr())  # count = 0: a no-op
    ctx.synchronize()
    got = o.cpu().numpy().reshape(M, 16)
    assert np.isfinite(got).all()
    clamped, _ = restate_hull(verts, wild, bodies, surface_lookup(tex, 4))
    np.testing.assert_array_equal(got, clamped)
    # the staged forms see the indices and refuse them
    for call in (ctx.body_hydrostatics, ctx.body_hydrostatics_async):
        with pytest.raises(oh.OceanError) as e:
            call(verts, wild, bodies)
        assert e.value.code == oh.E_INVALID_ARG
    with pytest.raises(oh.OceanError) as e:
        ctx.body_hydrostatics_device(vptr + 2, 300, dt.data_ptr(), 257, db.data_ptr(), M, o.data_ptr())
    assert e.value.code == oh.E_INVALID_ARG
    # count = 0: a no-op in the blocking form, but no request to hand back
    assert ctx.body_hydrostatics(verts, tris, np.zeros((0, 10), f32)).shape == (0, 16)
    with pytest.raises(oh.OceanError) as e:
        ctx.body_hydrostatics_async(verts, tris, np.zeros((0, 10), f32))
    assert e.value.code == oh.E_INVALID_ARG
    with pytest.raises(oh.OceanError) as e:
        ctx.body_hydrostatics(verts, tris, bodies, tile=1)
    assert e.value.code == oh.E_INVALID_ARG
    ctx.close()


def test_hull_state_and_kernel_kind():
    """OCEAN_E_STATE before ocean_init_spectrum; the launch is kind 2 of ocean_kernel_stats."""
    verts, tris = oh.OceanContext.box_mesh(1, 1, 1)
    bodies = np.zeros((1, 10), f32)
    bodies[:, 6], bodies[:, 7:10] = 1.0, 1.0
    ctx = oh.OceanContext(64, 1, 1)
    for call in (ctx.body_hydrostatics, ctx.body_hydrostatics_async):
        with pytest.raises(oh.OceanError) as e:
            call(verts, tris, bodies)
        assert e.value.code == oh.E_STATE
    ctx.close()
    ctx = make_ctx(64, O.SCENE_CASCADES[:1], times=())
    ctx.set_kernel_timing(True)
    before = ctx.kernel_stats(2)[1]
    ctx.body_hydrostatics(verts, tris, bodies)
    ctx.synchronize()
    assert ctx.kernel_stats(2)[1] == before + 1
    assert "k_body_hydrostatics" in ctx.kernel_name(2)
    ctx.close()


def test_hull_flat_water_is_archimedes():
    """Before the first ocean_step the water is flat at 0: the record is the float64 closed form (restate_hull in float64
    over flat water, which tests/test_hull_math.py holds to Archimedes at 1e-12) within 4 x the fp32 restatement's own
    rounding against float64, measured here, the camera tests' allowance; and it is the fp32 restatement bit for bit."""
    cas = O.SCENE_CASCADES[:2]
    ctx = make_ctx(64, cas, times=())
    rng = np.random.default_rng(77)
    size = 2.0
    verts, tris = oh.OceanContext.box_mesh(size, 0.5 * size, 0.75 * size, 3, 2, 4)
    bodies = poses(rng, size, 0.05 * size)
    got = ctx.body_hydrostatics(verts, tris, bodies)
    exact, m = restate_hull(verts.astype(np.float64), tris, bodies.astype(np.float64), flat, np.float64)
    fp32, _ = restate_hull(verts, tris, bodies, lambda q: np.zeros((len(q), 8), f32))
    np.testing.assert_array_equal(got, fp32)
    assert {0, 1, 2, 3} <= set(m.ravel())
    own = np.abs(fp32.astype(np.float64) - exact).max(axis=0)
    err = np.abs(got.astype(np.float64) - exact).max(axis=0)
    print("fp32 restatement against float64, per column:", " ".join(f"{x:.3g}" for x in own))
    print("kernel against float64, per column:          ", " ".join(f"{x:.3g}" for x in err))
    assert (err <= 4 * own).all()
    assert own.max() > 0  # the allowance is not vacuous
    vol = size * 0.5 * size * 0.75 * size * np.prod(bodies[:, 7:10].astype(np.float64), axis=1)
    # the deep body displaces its volume, the high one nothing.  104 terms of the size of depth x area, which cancel down
    # to the volume: a share of 1e-4 is some hundred roundings of the largest
    assert abs(got[0, 1] - vol[0]) <= 1e-4 * vol[0] and not got[4].any()
    np.testing.assert_array_equal(got[:, 7], np.zeros(M, f32))  # flat water: the fixed point is exact
    ctx.close()
