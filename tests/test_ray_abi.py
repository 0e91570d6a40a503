"""CPU tests of the ray casts and the surface bounds (ocean_raycast, _device, _async, ocean_surface_bounds, _device;
include/ocean/ocean.h): what can be checked without a GPU -- the symbols, the constants, the ctypes signatures,
the validation that precedes every device call, and restate_raycast, the numpy fp32 statement of a ray cast that
tests/test_gpu_ray.py compares the kernel with bit for bit.  The restatement is vectorised: it evaluates every
node of every ray, then picks the first crossing.  It has no air skip in it, so it is the single statement of the
result for both settings of OCEAN_RAY_BOUNDS.  Here it runs over oracle-made textures and on a flat sea, where
the answers are known."""
import ctypes

import numpy as np

import ocean_hip as oh
import oracle as O
from test_gpu_query import restate_surface

f32 = np.float32
RAY_SYMBOLS = ("ocean_surface_bounds", "ocean_surface_bounds_device", "ocean_raycast", "ocean_raycast_device",
               "ocean_raycast_async")


class OracleTextures:
    """DISP / DERIV / TURB [C][N][N][4] of one tile as arrays, with the S(p) of tests/test_gpu_query.py's Textures."""

    def __init__(self, disp, deriv, turb, cas):
        self.lengths = [c["wavelength"] for c in cas]
        self.disp, self.deriv, self.turb = disp, deriv, turb

    def _pts(self, p):
        return np.concatenate([p, np.zeros((len(p), 1), f32)], axis=1)

    def S(self, p):
        return O.sample_world(self.disp, self.deriv, self.turb, self.lengths, self._pts(p))

    def S_disp(self, p):
        return O.sample_world(self.disp, None, None, self.lengths, self._pts(p))[:, 0]


def ray_positions(rays, t):
    """pos(t) = o + t * d per component, one fp32 multiply and one fp32 add each: rays [M][8], t [M] -> [M][3]."""
    return rays[:, 0:3] + t[:, None] * rays[:, 3:6]


def _rec(tex, pos, k):
    """The OCEAN_QUERY_SURFACE record for the points (pos.x, pos.z) with k iterations, [M][8]."""
    return restate_surface(tex, np.ascontiguousarray(pos[:, [0, 2]]), (k,))[k]


def restate_raycast(tex, rays, k, steps, refine):
    """ocean.h's definition of ocean_raycast in numpy fp32, operation by operation: rays [M][8] -> [M][8]."""
    rays = np.ascontiguousarray(rays, f32)
    m = len(rays)
    t0, t1 = rays[:, 6], rays[:, 7]
    dt = (t1 - t0) / f32(steps)
    tn = t0[:, None] + np.arange(steps + 1, dtype=f32)[None, :] * dt[:, None]  # t_j, [M][S + 1]
    assert tn.dtype == f32
    pos = ray_positions(np.repeat(rays, steps + 1, axis=0), tn.ravel())
    f = (pos[:, 1] - _rec(tex, pos, k)[:, 0]).reshape(m, steps + 1)
    under = ~(f > 0)
    first = np.where(under.any(axis=1), under.argmax(axis=1), -1)  # the first node with !(f > 0), -1: none
    status = np.where(first == 0, oh.RAY_SUBMERGED, np.where(first > 0, oh.RAY_HIT, oh.RAY_MISS))
    tstar = np.where(first == 0, tn[:, 0], tn[:, steps]).astype(f32)
    hit = np.flatnonzero(first > 0)
    if len(hit):
        a, b = tn[hit, first[hit] - 1], tn[hit, first[hit]]
        for _ in range(refine):
            mid = f32(0.5) * (a + b)
            pm = ray_positions(rays[hit], mid)
            above = (pm[:, 1] - _rec(tex, pm, k)[:, 0]) > 0
            a, b = np.where(above, mid, a), np.where(above, b, mid)
        tstar[hit] = b
    pos = ray_positions(rays, tstar)
    r = _rec(tex, pos, k)
    out = np.empty((m, 8), f32)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = tstar, pos[:, 1] - r[:, 0], r[:, 3], status
    out[:, 4:] = r[:, 4:]
    return out


def _oracle_textures(n, cas, noise, t=1.0):
    disp, deriv, turb = O.OracleOcean(n, O.scene_params(), cas, noise).step(t)
    return OracleTextures(disp.astype(f32), deriv.astype(f32), turb.astype(f32), cas)


def test_ray_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in RAY_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.RAY_MISS, oh.RAY_HIT, oh.RAY_SUBMERGED) == (0, 1, 2)
    assert (oh.RAY_MAX_RAYS, oh.RAY_MAX_STEPS, oh.RAY_MAX_SAMPLES) == (16384, 1024, 1 << 24)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    ray = [P, i, i, i, i, P, i, P]
    want = {"ocean_surface_bounds": [P, i, P, sz], "ocean_surface_bounds_device": [P, i, P, sz],
            "ocean_raycast": ray, "ocean_raycast_device": ray, "ocean_raycast_async": ray + [ctypes.POINTER(P)]}
    for name, args in want.items():
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("surface_bounds", "surface_bounds_device", "raycast", "raycast_async", "raycast_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Raycast) and callable(oh.WaterBody.SurfaceBounds)


def test_ray_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    rays, out = np.zeros((2, 8), f32), np.zeros((2, 8), f32)
    args = (None, 0, 4, 16, 8, rays.ctypes.data, 2, out.ctypes.data)
    for name in ("ocean_raycast", "ocean_raycast_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*args) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)
    assert L.ocean_raycast_async(*args, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert b"context" in L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_raycast_async(*args, None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()
    for name in ("ocean_surface_bounds", "ocean_surface_bounds_device"):
        L.ocean_host_alloc(0, None)
        assert getattr(L, name)(None, 0, out.ctypes.data, 32) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    assert not out.any()


def test_flat_sea_known_answers():
    """Zero noise: no waves.  The ray (0, 5, 0) -> (0, -1, 0) over [0, 16] in 16 steps crosses on node 5: every
    bisection midpoint is above the water, so a climbs to 5 and t* = b = 5 exactly, with gap 0 and the normal
    (0, 1, 0).  From y = -1 the origin is under water; pointing up the ray never comes down."""
    n, cas = 32, O.SCENE_CASCADES[:2]
    tex = _oracle_textures(n, cas, np.zeros((n, n, 2), f32))
    assert not tex.disp[..., :3].any()  # (.w is the frame's constant 1)
    rays = f32([[0, 5, 0, 0, -1, 0, 0, 16], [0, -1, 0, 0, -1, 0, 0, 16], [0, 5, 0, 0, 1, 0, 0, 16],
                [3.5, 5, -7.25, 0, -1, 0, 0, 16]])
    for k in (0, 2):
        got = restate_raycast(tex, rays, k, 16, 8)
        np.testing.assert_array_equal(got[:, 3], f32([oh.RAY_HIT, oh.RAY_SUBMERGED, oh.RAY_MISS, oh.RAY_HIT]))
        np.testing.assert_array_equal(got[:, 0], f32([5, 0, 16, 5]))      # t*
        np.testing.assert_array_equal(got[:, 1], f32([0, -1, 21, 0]))     # gap
        np.testing.assert_array_equal(got[:, 2], f32([0, 0, 0, 0]))       # residual
        np.testing.assert_array_equal(got[:, 4:7], np.tile(f32([0, 1, 0]), (4, 1)))
    # without bisection the crossing node itself is returned; with fewer steps the bisection finds it
    np.testing.assert_array_equal(restate_raycast(tex, rays[:1], 0, 16, 0)[0, :4], f32([5, 0, 0, oh.RAY_HIT]))
    got = restate_raycast(tex, rays[:1], 0, 2, 3)  # nodes 0, 8, 16; [0, 8] -> 4, 6, 5
    np.testing.assert_array_equal(got[0, :4], f32([5, 0, 0, oh.RAY_HIT]))


def test_restatement_on_oracle_textures():
    """Over the oracle's own frame at N = 32: every record is consistent with the definition -- a hit ends at or
    under the water with the bracket's other end above it, a miss was above at every node, and the record's tail
    is the surface query's at the point met."""
    n, cas, k, steps, refine = 32, O.SCENE_CASCADES[:3], 2, 12, 6
    tex = _oracle_textures(n, cas, O.generate_noise(n, 20251121))
    top = float(np.abs(tex.disp[..., 1]).max(axis=(1, 2)).sum())
    assert top > 0
    rng = np.random.default_rng(5)
    m = 300
    rays = np.zeros((m, 8), f32)
    rays[:, [0, 2]] = rng.uniform(-2000, 2000, (m, 2))
    rays[:, 1] = rng.uniform(1.5 * top, 4 * top, m)
    rays[:, [3, 5]] = rng.uniform(-0.5, 0.5, (m, 2))
    rays[:, 4] = np.where(np.arange(m) % 3 == 0, 0.25, -1.0)  # a third climb: they miss
    rays[:, 7] = (rays[:, 1] + 2 * top) * 1.05
    rays[::7, 1] = -2 * top                                   # a seventh start under water
    out = restate_raycast(tex, rays, k, steps, refine)
    status = out[:, 3].astype(int)
    sub, up = np.arange(m) % 7 == 0, (np.arange(m) % 3 == 0)
    np.testing.assert_array_equal(status[sub], oh.RAY_SUBMERGED)
    np.testing.assert_array_equal(status[~sub & up], oh.RAY_MISS)
    np.testing.assert_array_equal(status[~sub & ~up], oh.RAY_HIT)
    hit = status == oh.RAY_HIT
    assert (out[hit, 1] <= 0).all() and (out[~sub & up, 1] > 0).all()
    dt = rays[:, 7] / steps
    t = out[:, 0]
    # more bisections only narrow the bracket from above: t* never grows, and moves by less than the bracket
    finer = restate_raycast(tex, rays[hit], k, steps, refine + 4)[:, 0]
    assert (finer <= t[hit]).all() and (t[hit] - finer <= dt[hit] / 2 ** refine * 1.001).all()
    np.testing.assert_array_equal(t[status == oh.RAY_MISS], (f32(steps) * dt)[status == oh.RAY_MISS])
    pos = ray_positions(rays, t)
    np.testing.assert_array_equal(out[:, 4:], _rec(tex, pos, k)[:, 4:])
    # the result is per ray: a subset gives the same rows
    np.testing.assert_array_equal(restate_raycast(tex, rays[10:20], k, steps, refine), out[10:20])
