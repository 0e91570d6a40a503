"""CPU tests of the buoyant-body entries (ocean_body_buoyancy, _device, _async; include/ocean/ocean.h): what
can be checked without a GPU -- the symbols, the constants, the validation that precedes every device call,
OceanContext.box_hull and buoyancy_wrench, and tree_sum, the numpy statement of the kernel's summation
order that tests/test_gpu_body.py builds its restatement on.  The kernel and the semantics are tested on the
GPU there."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh

BODY_SYMBOLS = ("ocean_body_buoyancy", "ocean_body_buoyancy_device", "ocean_body_buoyancy_async")
f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def segment_width(p):
    """W of ocean.h: the smallest power of two >= P, capped at 64."""
    w = 1
    while w < p and w < 64:
        w *= 2
    return w


def tree_sum(x):
    """The sum over the last axis (the P probes of a body) in the order ocean.h defines, in fp32: lane l < W
    adds its terms j = l, l + W, ... in ascending order onto +0, then the upper half of the lanes is folded
    onto the lower half until one is left."""
    x = np.asarray(x, f32)
    p = x.shape[-1]
    w = segment_width(p)
    t = np.zeros(x.shape[:-1] + (w,), f32)
    for j0 in range(0, p, w):
        chunk = x[..., j0:j0 + w]
        t[..., :chunk.shape[-1]] = t[..., :chunk.shape[-1]] + chunk
    while w > 1:
        w //= 2
        t = t[..., :w] + t[..., w:2 * w]
    return t[..., 0]


def test_body_symbols_exported():
    L = oh.load_library()
    for s in BODY_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.BODY_MAX_BODIES, oh.BODY_MAX_PROBES, oh.BODY_MAX_SAMPLES) == (8192, 4096, 1 << 22)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    for name in ("body_buoyancy", "body_buoyancy_async", "body_buoyancy_device", "box_hull", "buoyancy_wrench"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Buoyancy)


def test_body_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    hull, bodies, out = np.zeros((1, 5), f32), np.zeros((2, 10), f32), np.zeros((2, 8), f32)
    args = (None, 0, oh.QUERY_SURFACE, 4, hull.ctypes.data, 1, bodies.ctypes.data, 2, out.ctypes.data)
    for name in ("ocean_body_buoyancy", "ocean_body_buoyancy_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*args) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)
    assert L.ocean_body_buoyancy_async(*args, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert b"context" in L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_body_buoyancy_async(*args, None) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert not out.any()


def test_box_hull_lattice():
    """Cell centres of the unit box, x fastest, then z, then y; h = 1 / ny, v = 1 / (nx ny nz)."""
    h = oh.OceanContext.box_hull(2, 2)
    assert h.dtype == f32 and h.shape == (4, 5)
    np.testing.assert_array_equal(h, f32([[-0.25, 0, -0.25, 1, 0.25], [0.25, 0, -0.25, 1, 0.25],
                                          [-0.25, 0, 0.25, 1, 0.25], [0.25, 0, 0.25, 1, 0.25]]))
    h = oh.OceanContext.box_hull(4, 1)
    np.testing.assert_array_equal(h, f32([[-0.375, 0, 0, 1, 0.25], [-0.125, 0, 0, 1, 0.25],
                                          [0.125, 0, 0, 1, 0.25], [0.375, 0, 0, 1, 0.25]]))
    h = oh.OceanContext.box_hull(3, 2, ny=2)
    assert h.shape == (12, 5)
    xs = [f32((i + 0.5) / 3 - 0.5) for i in range(3)]
    assert xs[1] == 0.0 and xs[0] == -xs[2]
    for y, ry in enumerate((-0.25, 0.25)):
        for z, rz in enumerate((-0.25, 0.25)):
            for x in range(3):
                row = h[(y * 2 + z) * 3 + x]
                assert (row[0], row[1], row[2], row[3]) == (xs[x], f32(ry), f32(rz), f32(0.5)), (x, z, y)
                assert row[4] == f32(1.0 / 12.0)
    # the cells tile the box: volumes sum to 1, centres to 0
    assert abs(float(h[:, 4].astype(np.float64).sum()) - 1.0) < 12 * EPS32
    assert np.abs(h[:, :3].astype(np.float64).sum(axis=0)).max() < 12 * EPS32
    with pytest.raises(ValueError):
        oh.OceanContext.box_hull(0, 1)


@pytest.mark.parametrize("p", [1, 2, 3, 5, 8, 37, 64, 65, 130, 4096])
def test_tree_sum_is_a_sum(p):
    """Any summation order of P fp32 terms lies within (P - 1) eps sum |x| of the exact sum, to first order."""
    rng = np.random.default_rng(p)
    x = (rng.standard_normal((7, p)) * 10.0 ** rng.uniform(-3, 3, (7, p))).astype(f32)
    got = tree_sum(x).astype(np.float64)
    x64 = x.astype(np.float64)
    assert got.shape == (7,)
    assert (np.abs(got - x64.sum(axis=1)) <= p * EPS32 * np.abs(x64).sum(axis=1)).all()


def test_tree_sum_order_written_out():
    rng = np.random.default_rng(3)
    assert [segment_width(p) for p in (1, 2, 3, 4, 5, 37, 64, 65, 4096)] == [1, 2, 4, 4, 8, 64, 64, 64, 64]
    z = f32(0)
    x = (rng.standard_normal(3) * [1e4, 1.0, 1e-3]).astype(f32)  # W = 4: lanes (x0, x1, x2, +0)
    assert tree_sum(x) == ((z + x[0]) + (z + x[2])) + ((z + x[1]) + z)
    x = (rng.standard_normal(5) * [1e4, 1.0, 1e-3, 30.0, 1e2]).astype(f32)  # W = 8: lanes (x0 .. x4, +0, +0, +0)
    assert tree_sum(x) == ((x[0] + x[4]) + (x[2] + z)) + ((x[1] + z) + (x[3] + z))
    x = (rng.standard_normal(65) * 10.0 ** rng.uniform(-3, 3, 65)).astype(f32)  # W = 64: lane 0 holds x0 + x64
    lanes = [z + x[l] for l in range(64)]
    lanes[0] = lanes[0] + x[64]
    for s in (32, 16, 8, 4, 2, 1):
        lanes = [lanes[l] + lanes[l ^ s] for l in range(64)]  # the butterfly itself, every lane
    assert tree_sum(x) == lanes[0]
    assert len({float(v) for v in lanes}) == 1  # all lanes end with the same bits
    # the order matters in fp32: this is not the left-to-right sum in general
    y = f32([1.0, EPS32 / 2, EPS32 / 2])
    assert tree_sum(y) == f32(1.0) and (y[1] + y[2]) + y[0] != f32(1.0)
    assert tree_sum(f32([-0.0])) == 0.0 and not np.signbit(tree_sum(f32([-0.0])))  # +0 + -0 = +0


def test_buoyancy_wrench_hand_computed():
    """rho g out[0] along +y at out[1..3] / out[0]; torque about the origin r x F = rho g (-out[3], 0, out[1])."""
    out = f32([[2.0, 1.0, -3.0, 0.5, 0.1, 1.9, -0.2, 1e-4], [0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]])
    force, point, torque = oh.OceanContext.buoyancy_wrench(out, density=1000.0, gravity=10.0)
    np.testing.assert_array_equal(force, [[0.0, 20000.0, 0.0], [0.0, 0.0, 0.0]])
    np.testing.assert_array_equal(point, [[0.5, -1.5, 0.25], [0.0, 0.0, 0.0]])  # a dry body: no division by zero
    np.testing.assert_array_equal(torque, [[-5000.0, 0.0, 10000.0], [0.0, 0.0, 0.0]])
    np.testing.assert_allclose(np.cross(point[0], force[0]), torque[0], rtol=1e-15)
    f1, p1, t1 = oh.OceanContext.buoyancy_wrench(out[0], 1.0, 1.0)  # one record
    assert f1.shape == p1.shape == t1.shape == (1, 3) and f1[0, 1] == 2.0
