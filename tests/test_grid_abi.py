"""CPU tests of the surface-grid entries (ocean_surface_grid, _device, _async; include/ocean/ocean.h):
what can be checked without a GPU -- the symbols, the constants, the validation that precedes every
device call, the node arithmetic of OceanContext.grid_points and the hosts' surface.  The kernel and
the semantics are tested on the GPU in tests/test_gpu_grid.py."""
import ctypes

import numpy as np

import ocean_hip as oh

GRID_SYMBOLS = ("ocean_surface_grid", "ocean_surface_grid_device", "ocean_surface_grid_async")
f32 = np.float32


def test_grid_symbols_exported():
    L = oh.load_library()
    for s in GRID_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.GRID_VERTICES, oh.GRID_SURFACE, oh.GRID_HEIGHTFIELD, oh.GRID_MAX_NODES) == (0, 1, 2, 1 << 22)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)


def test_grid_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    out = np.zeros((2, 2, 8), f32)
    args = (None, 0, oh.GRID_SURFACE, 4, 0.0, 0.0, 0.0, 1.0, 1.0, 2, 2, out.ctypes.data, out.nbytes)
    for name in ("ocean_surface_grid", "ocean_surface_grid_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*args) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    assert L.ocean_surface_grid_async(*args, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_surface_grid_async(*args, None) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert not out.any()


def test_grid_points_written_out():
    """Node (i, j) = (x0 + float32(i) * dx, z0 + float32(j) * dz) at row j * nx + i, in fp32."""
    # MeshGenerator's defaults (MeshGenerator.cs:19-35): 101 vertices, 10 m apart, centred on the origin
    p = oh.OceanContext.grid_points(-500.0, -500.0, 10.0, 10.0, 101, 101)
    assert p.dtype == f32 and p.shape == (101 * 101, 2)
    g = p.reshape(101, 101, 2)
    want = np.arange(-500, 501, 10).astype(f32)  # integers: exact in fp32
    np.testing.assert_array_equal(g[0, :, 0], want)
    np.testing.assert_array_equal(g[:, 0, 1], want)
    np.testing.assert_array_equal(g[37, :, 0], want)  # x along the row, z constant in it
    np.testing.assert_array_equal(g[37, :, 1], np.full(101, -130.0, f32))
    np.testing.assert_array_equal(p[3 * 101 + 2], f32([-480.0, -470.0]))
    # a negative dx and a spacing that is not representable: the product is rounded, then the sum
    p = oh.OceanContext.grid_points(1.5, -2.0, -0.1, 0.3, 4, 3)
    assert p.shape == (12, 2)
    x = [f32(1.5), f32(1.5) + f32(1.0) * f32(-0.1), f32(1.5) + f32(2.0) * f32(-0.1), f32(1.5) + f32(3.0) * f32(-0.1)]
    z = [f32(-2.0), f32(-2.0) + f32(1.0) * f32(0.3), f32(-2.0) + f32(2.0) * f32(0.3)]
    for j in range(3):
        for i in range(4):
            assert p[j * 4 + i, 0] == x[i] and p[j * 4 + i, 1] == z[j], (i, j)
    assert p[7, 0] == p[3, 0] and p[3, 0] < p[2, 0] < p[1, 0] < p[0, 0] == f32(1.5)
    # the bits, from the definition in exact arithmetic: fl(-0.1) = -13421773 / 2^27, so node 1 is
    # 1.5 - 13421773 / 2^27 = 187904819 / 2^27, rounded to the 2^-23 grid of [1, 2): 11744051 / 2^23
    assert float(p[1, 0]) == 11744051 / 2.0 ** 23
    # z: doubling fl(0.3) is exact, so node 2 is -2 + 2 fl(0.3) rounded once
    assert float(p[8, 1]) == float(f32(-2.0) + f32(f32(0.3) + f32(0.3)))
    # zero spacing: every node of the axis coincides
    p = oh.OceanContext.grid_points(7.25, 1.0, 0.0, 2.0, 3, 2)
    np.testing.assert_array_equal(p, f32([[7.25, 1], [7.25, 1], [7.25, 1], [7.25, 3], [7.25, 3], [7.25, 3]]))


def test_host_surface_of_the_grids():
    assert callable(oh.OceanContext.surface_grid) and callable(oh.OceanContext.surface_grid_async)
    assert callable(oh.OceanContext.grid_points)
    assert callable(oh.WaterBody.SurfaceGrid)
    # iterations default to 4, to 0 for the vertices; the result's shape and size per mode
    assert oh.OceanContext._grid_args(oh.GRID_SURFACE, None, 5, 3) == (4, (3, 5, 8), 480)
    assert oh.OceanContext._grid_args(oh.GRID_VERTICES, None, 5, 3) == (0, (3, 5, 8), 480)
    assert oh.OceanContext._grid_args(oh.GRID_HEIGHTFIELD, 16, 5, 3) == (16, (3, 5), 60)
