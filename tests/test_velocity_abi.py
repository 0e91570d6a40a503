"""CPU tests of the surface velocity (OCEAN_F_VELOCITY, OCEAN_TEX_VELOCITY, ocean_query_velocity, _device, _async;
include/ocean/ocean.h): what can be checked without a GPU -- the symbols, the constants, the validation that
precedes every device call, and velocity_planes, the numpy fp32 statement of the two packed planes of dh/dt
that tests/test_gpu_velocity.py compares the VELOCITY texture with.  The definition itself is checked here against
the oracle: the transform of velocity_planes must be the time derivative of the oracle's own DISP."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O

VELOCITY_SYMBOLS = ("ocean_query_velocity", "ocean_query_velocity_device", "ocean_query_velocity_async")
f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def velocity_planes(h0, waves, t, leak=True):
    """ocean.h's definition in numpy fp32, operation by operation: h0, waves float32[C][N][N][4] -> (V0, V1),
    float32[C][N][N][2] each, the DxDz / DyDxz packing of dh/dt = i omega (A - B) at time t.  (cos, sin) are
    numpy's fp32 ones where the library runs its own 1-2 ulp pair.  leak=False drops the Dxz term of V1 (the
    "clean" packing, which is NOT the derivative of this library's DISP.y; kept to show the check sees it)."""
    h0, w, t = np.asarray(h0, f32), np.asarray(waves, f32), f32(t)
    hx, hy, hz, hw = (h0[..., k] for k in range(4))
    wx, wy, wz, om = (w[..., k] for k in range(4))
    phase = om * t
    ex, ey = np.cos(phase), np.sin(phase)
    assert ex.dtype == f32
    ax, ay = hx * ex - hy * ey, hx * ey + hy * ex
    bx, by = hz * ex - hw * (-ey), hz * (-ey) + hw * ex
    gx, gy = ax - bx, ay - by
    tx, ty = -(gy * om), gx * om                       # ht = i omega (A - B)
    ihx, ihy = -ty, tx
    dx_x, dx_y = (ihx * wx) * wy, (ihy * wx) * wy
    dz_x, dz_y = (ihx * wz) * wy, (ihy * wz) * wy
    aux_x, aux_y = -tx * wy, -ty * wy
    dzdx_x, dzdx_y = aux_x * wx * wz, aux_y * wx * wz
    v0 = np.stack([dx_x - dz_y, dx_y + dz_x], axis=-1)
    v1 = np.stack([tx - dzdx_y, ty + dzdx_x], axis=-1) if leak else np.stack([tx, ty], axis=-1)
    return v0.astype(f32), v1.astype(f32)


def velocity_texture(h0, waves, t, leak=True):
    """VEL float32[C][N][N][4] = (Re V0, Re V1, Im V0, Im V1) of the transformed planes (the oracle's operator)."""
    v0, v1 = velocity_planes(h0, waves, t, leak)
    a, b = O.ifft2d(v0), O.ifft2d(v1)
    return np.stack([a[..., 0], b[..., 0], a[..., 1], b[..., 1]], axis=-1)


def finite_difference_bound(omega_max, t, dt):
    """Norm-relative error allowed between VEL and the central difference of DISP at t +- dt: the difference's
    truncation for the fastest wave, (omega dt)^2 / 6, plus the fp32 rounding of DISP and of the phase omega t,
    both amplified by 1 / dt: 4 eps (1 + t) / dt."""
    return (float(omega_max) * dt) ** 2 / 6.0 + 4.0 * EPS32 * (1.0 + t) / dt


def test_velocity_symbols_and_constants():
    L = oh.load_library()
    for s in VELOCITY_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.F_VELOCITY, oh.TEX_VELOCITY) == (0x10, 11)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    for name in ("query_velocity", "query_velocity_async", "query_velocity_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.GetWaterVelocity)
    assert oh.WaterBody().velocity is False


def test_velocity_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    pts, out = np.zeros((2, 2), f32), np.zeros((2, 8), f32)
    args = (None, 0, 4, pts.ctypes.data, 2, out.ctypes.data)
    for name in ("ocean_query_velocity", "ocean_query_velocity_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*args) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)
    assert L.ocean_query_velocity_async(*args, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert b"context" in L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_query_velocity_async(*args, None) == oh.E_INVALID_ARG
    assert L.ocean_last_error()
    assert not out.any()


def _spectrum(n, ncasc, shallow):
    return O.init_spectrum(n, O.scene_params(shallow), O.SCENE_CASCADES[:ncasc], O.generate_noise(n, 20251121))


def _central_difference(h0, w, t, dt):
    def disp(tt):
        planes = O.evolve(h0, w, tt)
        d, _, _ = O.fill([O.ifft2d(planes[0]), O.ifft2d(planes[1])], full=False)
        return d.astype(np.float64)
    return (disp(t + dt) - disp(t - dt)) / (2.0 * dt)


CASES = [(16, 1, False), (64, 2, False), (64, 4, False), (128, 3, True)]


@pytest.mark.parametrize("n,ncasc,shallow", CASES)
def test_velocity_is_the_time_derivative_of_disp(n, ncasc, shallow):
    """VEL.xyz from velocity_planes against the central difference of the oracle's DISP.xyz, per cascade and
    channel, at t = 1, dt = 1 / 64 (exact in fp32).  A wrong sign or factor gives O(1)."""
    t, dt = 1.0, 1.0 / 64.0
    h0, w = _spectrum(n, ncasc, shallow)
    vel = velocity_texture(h0, w, t)
    fd = _central_difference(h0, w, t, dt)
    for c in range(ncasc):
        bound = finite_difference_bound(w[c, ..., 3].max(), t, dt)
        for ch, name in enumerate("xyz"):
            e = O.rel_err(vel[c, ..., ch], fd[c, ..., ch])
            print(f"N = {n}, cascade {c}, {name}: rel err {e:.3e}, bound {bound:.3e}")
            assert e <= bound, (n, c, name, e, bound)


def test_the_check_rejects_the_clean_packing():
    """Without the Dxz term in V1, Re V1 is not the derivative of this library's DISP.y (the reference's spectrum
    is not Hermitian on its Nyquist row and column, so DISP.y carries a leak of Dxz): the condition above must
    see that, or it would not tell the two definitions apart."""
    t, dt = 1.0, 1.0 / 64.0
    n, ncasc = 64, 2
    h0, w = _spectrum(n, ncasc, False)
    vel = velocity_texture(h0, w, t, leak=False)
    fd = _central_difference(h0, w, t, dt)
    worst = max(O.rel_err(vel[c, ..., 1], fd[c, ..., 1]) / finite_difference_bound(w[c, ..., 3].max(), t, dt)
                for c in range(ncasc))
    print(f"clean packing: worst y error / bound = {worst:.1f}")
    assert worst > 1.0


def test_out_of_band_texels_are_zero():
    """omega = 0 outside the band: both planes vanish there."""
    n = 64
    h0, w = O.init_spectrum(n, O.scene_params(), [dict(O.SCENE_CASCADES[3])], O.generate_noise(n, 3))
    out = w[..., 3] == 0
    assert out.any() and not out.all()
    v0, v1 = velocity_planes(h0, w, 1.0)
    assert not v0[out].any() and not v1[out].any()
    assert v0[~out].any() and v1[~out].any()
