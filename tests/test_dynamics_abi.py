"""CPU tests of the body-dynamics entries (ocean_body_dynamics, _device, _async; include/ocean/ocean.h): what can
be checked without a GPU -- the symbols, the constants, the validation that precedes every device call -- and
restate_dynamics, the numpy fp32 statement of the kernel's per-probe terms and sums that
tests/test_gpu_dynamics.py compares the kernel with bit for bit, itself checked here against a wrench computed
by hand."""
import ctypes

import numpy as np

import ocean_hip as oh
from test_body_abi import tree_sum
from test_gpu_body import body_geometry, cross

DYNAMICS_SYMBOLS = ("ocean_body_dynamics", "ocean_body_dynamics_device", "ocean_body_dynamics_async")
f32 = np.float32


def probe_points(hull, bodies):
    """q float32[M * P][2]: the world (x, z) of every probe, body-major, where the lookups are taken."""
    _, w, _, _ = body_geometry(hull, bodies)
    return np.stack([w[0].ravel(), w[2].ravel()], axis=1)


def restate_dynamics(hull, bodies, motion, law, rec, vs):
    """ocean_body_dynamics in numpy fp32, in ocean.h's operation order.  rec float32[M * P][8]: per probe the record
    the mode defines at probe_points (height, -, -, r, n, -); vs float32[M * P][>= 3]: the water's velocity there
    (Vs(p_K), or the picked texel of VEL in reference mode).  Returns (out float32[M][16], f float32[M][P])."""
    m, p = len(bodies), len(hull)
    d, w, hs, vol = body_geometry(hull, bodies)
    rec = np.asarray(rec, f32).reshape(m, p, 8)
    vs = np.asarray(vs, f32).reshape(m, p, -1)
    mo = np.asarray(motion, f32)[:, None, :]
    eta, r, n = rec[..., 0], rec[..., 3], rec[..., 4:7]
    half, zero, one = f32(0.5), f32(0.0), f32(1.0)
    bottom = w[1] - half * hs
    f = np.minimum(np.maximum((eta - bottom) / hs, zero), one)
    g = vol * f
    e = (d[0], (d[1] - half * hs) + half * (f * hs), d[2])
    oxe = cross((mo[..., 3], mo[..., 4], mo[..., 5]), e)
    u = tuple(vs[..., i] - (mo[..., i] + oxe[i]) for i in range(3))
    mag = np.sqrt((u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])
    assert mag.dtype == f32
    s = g * mag if law == oh.DRAG_QUADRATIC else g
    force = tuple(s * u[i] for i in range(3))
    torque = cross(e, force)
    wet = f > zero
    terms = [g, g * e[0], g * e[1], g * e[2], g * n[..., 0], g * n[..., 1], g * n[..., 2], None,
             force[0], force[1], force[2], torque[0], torque[1], torque[2], None, wet.astype(f32)]
    out = np.empty((m, 16), f32)
    for k, term in enumerate(terms):
        if term is not None:
            out[:, k] = tree_sum(term)
    out[:, 7] = r.max(axis=1)
    out[:, 14] = np.where(wet, mag, zero).max(axis=1)
    return out, f


def test_dynamics_symbols_exported():
    L = oh.load_library()
    for s in DYNAMICS_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.DRAG_LINEAR, oh.DRAG_QUADRATIC) == (0, 1)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    for name in ("body_dynamics", "body_dynamics_async", "body_dynamics_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Dynamics)


def test_dynamics_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    hull, bodies, motion, out = np.zeros((1, 5), f32), np.zeros((2, 10), f32), np.zeros((2, 6), f32), np.zeros((2, 16), f32)
    args = (None, 0, oh.QUERY_SURFACE, 4, oh.DRAG_LINEAR, hull.ctypes.data, 1, bodies.ctypes.data, motion.ctypes.data, 2,
            out.ctypes.data)
    for name in ("ocean_body_dynamics", "ocean_body_dynamics_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*args) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)
    assert L.ocean_body_dynamics_async(*args, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert b"context" in L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_body_dynamics_async(*args, None) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert not out.any()


def test_restatement_against_a_hand_computed_wrench():
    """One body at the origin, identity pose, unit scale; two probes of height 2 at x = +-1 (W = 2: lane 0 + lane 1).
    Probe 0: eta = 0 -> bottom -1, f = 1/2, g = 1/2, e = (1, -1/2, 0).  Probe 1: eta = 1 -> f = 1, g = 1/2, e = (-1, 0, 0).
    Motion v = (0, 0, 1), omega = (0, 1, 0): omega x e = (e.z, 0, -e.x), so vb = (0, 0, 0) and (0, 0, 2).
    Water (1, 0, 0) and (0, 3, 6): u = (1, 0, 0), m = 1 and u = (0, 3, 4), m = 5.
    Linear: F = (1/2, 0, 0) and (0, 3/2, 2); T = e x F = (0, 0, 1/4) and (0, 2, -3/2).
    Quadratic: probe 0 as before (m = 1); probe 1 s = 5/2, F = (0, 15/2, 10), T = (0, 10, -15/2)."""
    hull = f32([[1, 0, 0, 2, 1], [-1, 0, 0, 2, 0.5]])
    bodies = f32([[0, 0, 0, 0, 0, 0, 1, 1, 1, 1]])
    motion = f32([[0, 0, 1, 0, 1, 0]])
    np.testing.assert_array_equal(probe_points(hull, bodies), f32([[1, 0], [-1, 0]]))
    rec = f32([[0, 9, 9, 0.25, 0, 1, 0, 9], [1, 9, 9, 0.5, 0, 1, 0, 9]])
    vs = f32([[1, 0, 0, 7], [0, 3, 6, 7]])
    buoyancy = [1.0, 0.0, -0.25, 0.0, 0.0, 1.0, 0.0, 0.5]
    out, f = restate_dynamics(hull, bodies, motion, oh.DRAG_LINEAR, rec, vs)
    assert out.dtype == f32 and out.shape == (1, 16)
    np.testing.assert_array_equal(f, f32([[0.5, 1.0]]))
    np.testing.assert_array_equal(out[0], f32(buoyancy + [0.5, 1.5, 2.0, 0.0, 2.0, -1.25, 5.0, 2.0]))
    out, _ = restate_dynamics(hull, bodies, motion, oh.DRAG_QUADRATIC, rec, vs)
    np.testing.assert_array_equal(out[0], f32(buoyancy + [0.5, 7.5, 10.0, 0.0, 10.0, -7.25, 5.0, 2.0]))
    # probe 1 lifted out of the water (eta = -5): g = 0 through the formulas, so it adds +-0 to every sum, is not
    # counted, and its relative speed of 5 does not enter out[14]
    rec[1, 0] = -5.0
    for law in (oh.DRAG_LINEAR, oh.DRAG_QUADRATIC):
        out, f = restate_dynamics(hull, bodies, motion, law, rec, vs)
        np.testing.assert_array_equal(f, f32([[0.5, 0.0]]))
        np.testing.assert_array_equal(out[0], f32([0.5, 0.5, -0.25, 0.0, 0.0, 0.5, 0.0, 0.5,
                                                   0.5, 0.0, 0.0, 0.0, 0.0, 0.25, 1.0, 1.0]))
