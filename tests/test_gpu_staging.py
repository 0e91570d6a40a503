"""GPU tests of the staging that the point consumers share (csrc/abi_readback.cpp: the one blocking staging
block, the one async slot layout): what no consumer's own suite pins.  Each consumer's results are tested bit
for bit against the numpy restatements elsewhere (tests/test_gpu_query.py and its siblings); here the forms
are compared with one another, bit for bit, on one small context."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_body import random_bodies, random_hull
from test_gpu_dynamics import random_motion
from test_gpu_query import make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
N, CAS = 64, O.SCENE_CASCADES[:2]


def points(rng, m):
    return rng.uniform(-200.0, 200.0, (m, 2)).astype(f32)


def test_async_requests_of_every_consumer_reuse_one_slot():
    """A surface query (M = 5), bodies (P = 3, M = 4), a velocity query (M = 7), a 3 x 2 surface grid, dynamics
    (P = 3, M = 4), a surface query (M = 1), a ray cast (M = 5) and the whitecaps of the 3 x 2 grid, each issued,
    read and released before the next, so that every request takes the pool's one slot: the pinned input copy
    and the device layout behind the results are shared, and no request leaves anything behind for the next.
    The dynamics request lays its inputs out right behind its own records, the query after it at the point
    queries' offset in the same slot.  Each equals its blocking form bit for bit."""
    ctx = make_ctx(N, CAS, oh.F_VELOCITY)
    rng = np.random.default_rng(20251121)
    q5, q7, q1 = points(rng, 5), points(rng, 7), points(rng, 1)
    hull, bodies = random_hull(rng, 3, 2.0), random_bodies(rng, 4, 1.0, span=200.0)
    motion = random_motion(rng, 4, 1.0)
    grid = (-5.0, 3.5, 1.3, 0.7, 3, 2)
    rays = np.zeros((5, 8), f32)  # straight down from 50 m up: every ray meets the water
    rays[:, [0, 2]] = points(rng, 5)
    rays[:, 1], rays[:, 4], rays[:, 7] = 50.0, -1.0, 100.0
    caps = (-1e30, *grid)  # every node is selected
    records = lambda rb: rb.data  # noqa: E731
    want = [ctx.query_surface(q5), ctx.body_buoyancy(hull, bodies), ctx.query_velocity(q7),
            ctx.surface_grid(*grid, mode=oh.GRID_SURFACE), ctx.body_dynamics(hull, bodies, motion),
            ctx.query_surface(q1), ctx.raycast(rays), ctx.whitecaps(*caps, capacity=7)[1]]
    issue = [(lambda: ctx.query_surface_async(q5), records), (lambda: ctx.body_buoyancy_async(hull, bodies), records),
             (lambda: ctx.query_velocity_async(q7), records),
             (lambda: ctx.surface_grid_async(*grid, mode=oh.GRID_SURFACE), records),
             (lambda: ctx.body_dynamics_async(hull, bodies, motion), records),
             (lambda: ctx.query_surface_async(q1), records), (lambda: ctx.raycast_async(rays), records),
             (lambda: ctx.whitecaps_async(*caps, capacity=7), lambda rb: rb.whitecaps()[1])]
    assert want[-1].shape == (6, 8)
    for k, ((request, read), expected) in enumerate(zip(issue, want)):
        rb = request()
        got = read(rb)
        rb.release()
        assert np.isfinite(got).all() and got.any(), k
        np.testing.assert_array_equal(got, expected, err_msg=f"request {k}")
    ctx.close()


def test_rejections_follow_the_order_of_each_form():
    """What each form of a consumer tests first, on a context created with OCEAN_F_VELOCITY whose spectrum was never
    initialised, so that every call is rejected and no consumer kernel runs (no buffer is read either: the pointers
    are host addresses).  Each row is a call, its code and a part of ocean_last_error.  The blocking forms test the
    context's state before they return for an empty call; the async forms refuse an empty call before they look at
    the state, and leave *req NULL; the _device forms test alignment before the state and have no staging limit;
    whitecaps test alignment before the tile, grids the tile before alignment; the flag precedes the state; and a
    grid larger than a readback slot (N = 64: 65536 x 40 B = 81920 nodes of 32 B) is refused by the async form."""
    ctx, plain = oh.OceanContext(N, len(CAS), 1, oh.F_VELOCITY), oh.OceanContext(N, len(CAS), 1)
    L, h = ctx.lib, ctx._h
    buf = np.zeros(64, f32)
    a = (buf.ctypes.data + 15) & ~15  # 16-byte aligned, and a + 4 is not
    S, K, lin = oh.QUERY_SURFACE, 4, oh.DRAG_LINEAR
    region, big = (0.0, 0.0, 1.0, 1.0, 3, 2), (0.0, 0.0, 1.0, 1.0, 1, 81921)
    # the arguments of each family's host form as functions of (context, count or tile, out)
    host = {
        "query_surface": lambda c, m, o: (c, 0, S, K, a, m, o),
        "query_velocity": lambda c, m, o: (c, 0, K, a, m, o),
        "body_buoyancy": lambda c, m, o: (c, 0, S, K, a, 1, a, m, o),
        "body_dynamics": lambda c, m, o: (c, 0, S, K, lin, a, 1, a, a, m, o),
        "raycast": lambda c, m, o: (c, 0, K, 1, 0, a, m, o),
    }
    grid = lambda c, t, o, r=region: (c, t, oh.GRID_SURFACE, K, 0.0, *r, o, r[4] * r[5] * 32)  # noqa: E731
    caps = lambda c, t, o: (c, t, 0.0, 0.5, *region, 7, o, 8 * 32)  # noqa: E731
    limits = {"query_surface": ("QUERY_MAX_POINTS", oh.QUERY_MAX_POINTS), "body_buoyancy": ("BODY_MAX_BODIES", oh.BODY_MAX_BODIES),
              "raycast": ("RAY_MAX_RAYS", oh.RAY_MAX_RAYS)}
    rows = []  # (what, entry, arguments, code, part of the message)
    for name, args in host.items():
        rows.append((f"{name}, empty", f"ocean_{name}", args(h, 0, a), oh.E_STATE, "must precede"))
        rows.append((f"{name}_async, empty", f"ocean_{name}_async", args(h, 0, a), oh.E_INVALID_ARG, "so no request"))
        rows.append((f"{name}_device, out + 4", f"ocean_{name}_device", args(h, 3, a + 4), oh.E_INVALID_ARG, "aligned"))
    for name, (limit, m) in limits.items():
        rows.append((f"{name}_device over the limit", f"ocean_{name}_device", host[name](h, m + 1, a), oh.E_STATE, "must precede"))
        rows.append((f"{name} over the limit", f"ocean_{name}", host[name](h, m + 1, a), oh.E_INVALID_ARG, limit))
    for name, args in (("surface_grid", grid), ("whitecaps", caps)):
        rows.append((name, f"ocean_{name}", args(h, 0, a), oh.E_STATE, "must precede"))
        rows.append((f"{name}_async", f"ocean_{name}_async", args(h, 0, a), oh.E_STATE, "must precede"))
        rows.append((f"{name}_device, out + 4", f"ocean_{name}_device", args(h, 0, a + 4), oh.E_INVALID_ARG, "aligned"))
    rows.append(("whitecaps_device, out + 4 and tile 1", "ocean_whitecaps_device", caps(h, 1, a + 4), oh.E_INVALID_ARG, "aligned"))
    rows.append(("surface_grid_device, out + 4 and tile 1", "ocean_surface_grid_device", grid(h, 1, a + 4), oh.E_INVALID_ARG,
                 "tile out of range"))
    rows.append(("query_velocity without the flag", "ocean_query_velocity", host["query_velocity"](plain._h, 3, a),
                 oh.E_UNSUPPORTED, "OCEAN_F_VELOCITY"))
    rows.append(("body_dynamics without the flag", "ocean_body_dynamics", host["body_dynamics"](plain._h, 3, a),
                 oh.E_UNSUPPORTED, "OCEAN_F_VELOCITY"))
    rows.append(("surface_grid_async above a slot", "ocean_surface_grid_async", grid(h, 0, a, big), oh.E_INVALID_ARG,
                 "exceed a readback slot"))
    assert big[4] * big[5] <= oh.GRID_MAX_NODES and len(rows) == 32
    for what, entry, args, code, part in rows:
        if entry.endswith("_async"):
            req = ctypes.c_void_p(0x1234)
            rc = getattr(L, entry)(*args, ctypes.byref(req))
            assert req.value is None, what
        else:
            rc = getattr(L, entry)(*args)
        msg = L.ocean_last_error().decode()
        assert rc == code and part in msg, (what, rc, msg)
    ctx.close()
    plain.close()


def device_buffers(ctx, *arrays, out_floats):
    import torch
    dev = torch.device("cuda", ctx.device)
    bufs = [torch.from_numpy(np.ascontiguousarray(a).ravel()).to(dev) for a in arrays]
    out = torch.zeros(out_floats, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    return bufs, out


def test_counts_at_the_edges_of_the_staging_layout():
    """The blocking form stages its inputs at the base of one block and its output at the next 256-byte
    boundary; the async form stages them behind the slot's results.  Surface queries of M = 31, 32 and 33
    points are 248, 256 and 264 B of inputs (just under, on and just over the boundary); bodies with (M, P) =
    (6, 1) and (1, 13) are 240 + 20 = 260 B and 40 + 260 = 300 B, two arrays back to back whose sum crosses
    it.  Both forms equal the _device form over device buffers, bit for bit."""
    ctx = make_ctx(N, CAS)
    rng = np.random.default_rng(7)
    vp = ctypes.c_void_p
    for m in (31, 32, 33):
        q = points(rng, m)
        (dq,), out = device_buffers(ctx, q, out_floats=m * 8)
        assert ctx.lib.ocean_query_surface_device(ctx._h, 0, oh.QUERY_SURFACE, 4, vp(dq.data_ptr()), m,
                                                  vp(out.data_ptr())) == oh.OK
        ctx.synchronize()
        want = out.cpu().numpy().reshape(m, 8)
        assert np.isfinite(want).all() and want.any(), m
        np.testing.assert_array_equal(ctx.query_surface(q), want, err_msg=f"blocking, M = {m}")
        rb = ctx.query_surface_async(q)
        np.testing.assert_array_equal(rb.data, want, err_msg=f"async, M = {m}")
        rb.release()
    for m, p in ((6, 1), (1, 13)):
        hull, bodies = random_hull(rng, p, 2.0), random_bodies(rng, m, 1.0, span=200.0)
        (dh, db), out = device_buffers(ctx, hull, bodies, out_floats=m * 8)
        ctx.body_buoyancy_device(dh.data_ptr(), p, db.data_ptr(), m, out.data_ptr())
        ctx.synchronize()
        want = out.cpu().numpy().reshape(m, 8)
        assert np.isfinite(want).all() and want.any(), (m, p)
        np.testing.assert_array_equal(ctx.body_buoyancy(hull, bodies), want, err_msg=f"blocking, (M, P) = {(m, p)}")
        rb = ctx.body_buoyancy_async(hull, bodies)
        np.testing.assert_array_equal(rb.data, want, err_msg=f"async, (M, P) = {(m, p)}")
        rb.release()
    ctx.close()
