"""GPU tests of the staging that the point consumers share (csrc/ocean_abi.cpp: the one blocking staging
block, the one async slot layout): what no consumer's own suite pins.  Each consumer's results are tested bit
for bit against the numpy restatements elsewhere (tests/test_gpu_query.py and its siblings); here the forms
are compared with one another, bit for bit, on one small context."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_body import random_bodies, random_hull
from test_gpu_query import make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
N, CAS = 64, O.SCENE_CASCADES[:2]


def points(rng, m):
    return rng.uniform(-200.0, 200.0, (m, 2)).astype(f32)


def test_async_requests_of_every_consumer_reuse_one_slot():
    """A surface query (M = 5), bodies (P = 3, M = 4), a velocity query (M = 7), a 3 x 2 surface grid and a
    surface query (M = 1), each issued, read and released before the next, so that every request takes the
    pool's one slot: the pinned input copy and the device layout behind the results are shared, and no
    request leaves anything behind for the next.  Each equals its blocking form bit for bit."""
    ctx = make_ctx(N, CAS, oh.F_VELOCITY)
    rng = np.random.default_rng(20251121)
    q5, q7, q1 = points(rng, 5), points(rng, 7), points(rng, 1)
    hull, bodies = random_hull(rng, 3, 2.0), random_bodies(rng, 4, 1.0, span=200.0)
    grid = (-5.0, 3.5, 1.3, 0.7, 3, 2)
    want = [ctx.query_surface(q5), ctx.body_buoyancy(hull, bodies), ctx.query_velocity(q7),
            ctx.surface_grid(*grid, mode=oh.GRID_SURFACE), ctx.query_surface(q1)]
    issue = [lambda: ctx.query_surface_async(q5), lambda: ctx.body_buoyancy_async(hull, bodies),
             lambda: ctx.query_velocity_async(q7), lambda: ctx.surface_grid_async(*grid, mode=oh.GRID_SURFACE),
             lambda: ctx.query_surface_async(q1)]
    for k, (request, expected) in enumerate(zip(issue, want)):
        rb = request()
        got = rb.data
        rb.release()
        assert np.isfinite(got).all() and got.any(), k
        np.testing.assert_array_equal(got, expected, err_msg=f"request {k}")
    ctx.close()


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
