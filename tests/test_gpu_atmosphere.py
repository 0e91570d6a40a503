"""GPU tests of the atmosphere (ocean_atmosphere, ocean_sky_update, ocean_atmosphere_read / _lut, ocean_sun_color;
csrc/atmosphere.hip) against tests/atmosphere_ref.py, the numpy restatement of include/ocean/ocean.h.

The criterion, per table and colour channel: the device's norm-relative error against the float64 restatement is at
most 4 x the fp32 restatement's own error against float64 (the margin of the camera's colour test).  Both errors are
divided by the same norm, so the test compares the two distances themselves; where float64 and the fp32 restatement
agree exactly (a table that is zero), so must the device.  The fourth channel is exact.  The transmittance and the
multiscatter table are asserted whole; the sky-view table on every texel whose ray does not end on the planet in the
float64 restatement, the rest (ill-conditioned in the reference's own fp32, ocean.h) being asserted finite; the
unasserted share is printed and is at most half the rows.

Sizes: (8,16, 8,8, 16,8), a tile or less each; (12,20, 3,5, 20,12), no multiple of a tile and more than one
workgroup along both axes of the transmittance and the sky-view table; (2,2, 2,2, 2,2), the smallest allowed; and
AtmosphereController's defaults once.  Suns: high, on the horizon (y = 0), just below it (the upper air is still lit),
well below it (a black sky), the exact zenith, and a vector that is not normalised."""
import ctypes
import functools

import numpy as np
import pytest

import atmosphere_ref as A
import ocean_hip as oh

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
PARAMS = oh.atmosphere_params(ground_albedo=(0.3, 0.3, 0.3))  # the ground term is not zero
SMALL = [(8, 16, 8, 8, 16, 8), (12, 20, 3, 5, 20, 12), (2, 2, 2, 2, 2, 2)]
SUNS = [(0.3, 0.8, 0.2), (1.0, 0.0, 0.5), (0.6, -0.02, 0.3), (0.5, -0.3, 0.2), (0.0, 1.0, 0.0), (3.0, 4.0, 12.0)]


@functools.lru_cache(maxsize=None)
def reference_tm(dims, params=PARAMS.tobytes()):
    """{dtype: (T, M)} of the restatement, computed once per size and left unchanged."""
    p = np.frombuffer(params, f32)
    out = {}
    for t in (f32, np.float64):
        T = A.transmittance(p, dims[0], dims[1], t)
        M = A.multiscatter(p, T, dims[2], dims[3], t)
        T.setflags(write=False), M.setflags(write=False)
        out[t] = (T, M)
    return out


def reference_sky(dims, sun, params=PARAMS):
    """(S fp32, S float64, the texels whose ray ends on the planet in float64)."""
    ref = reference_tm(dims, params.tobytes())
    s32, _ = A.skyview(params, *ref[f32], sun, dims[4], dims[5], f32)
    s64, ends = A.skyview(params, *ref[np.float64], sun, dims[4], dims[5], np.float64)
    return s32, s64, ends


def check_table(name, dev, r32, r64, keep=None):
    """The criterion over the texels `keep` (all when None); returns the ratios device error / restatement error."""
    assert dev.dtype == f32 and dev.shape == r64.shape and np.isfinite(dev).all(), name
    np.testing.assert_array_equal(dev[..., 3], r64[..., 3].astype(f32), err_msg=name + ".w")
    keep = np.ones(dev.shape[:2], bool) if keep is None else keep
    ratios = []
    for c in range(3):
        ref = r64[..., c][keep]
        e_dev = np.linalg.norm(dev[..., c][keep].astype(np.float64) - ref)
        e_ref = np.linalg.norm(r32[..., c][keep].astype(np.float64) - ref)
        norm = np.linalg.norm(ref)
        print(f"{name} channel {c}: |ref| {norm:.6g}, restatement error {e_ref:.3g}, device error {e_dev:.3g}, "
              f"ratio {e_dev / e_ref if e_ref > 0 else 0.0:.3f}")
        assert e_dev <= 4.0 * e_ref, (name, c, e_dev, e_ref, norm)
        ratios.append(e_dev / e_ref if e_ref > 0 else 0.0)
    return ratios


def check_sky(dims, sun, dev):
    s32, s64, ends = reference_sky(dims, sun)
    rows = ends.any(axis=1)
    print(f"sky view {dims[4]} x {dims[5]}, sun {sun}: {int(rows.sum())} of {len(rows)} rows end on the planet (finite only)")
    assert 2 * rows.sum() <= len(rows)
    return check_table(f"sky view, sun {sun}", dev, s32, s64, ~ends)


def fresh(dims=None, params=PARAMS):
    ctx = oh.OceanContext(64, 1, 1)  # no spectrum: the atmosphere needs none
    ctx.atmosphere(params, dims)
    return ctx


@pytest.mark.parametrize("dims", SMALL)
def test_tables_match_the_restatement(dims):
    ctx = fresh(dims)
    ref = reference_tm(dims)
    T, M = ctx.atmosphere_lut(oh.LUT_TRANSMITTANCE), ctx.atmosphere_lut(oh.LUT_MULTISCATTER)
    assert T.shape == (dims[1], dims[0], 4) and M.shape == (dims[3], dims[2], 4)
    check_table("transmittance", T, ref[f32][0], ref[np.float64][0])
    check_table("multiscatter", M, ref[f32][1], ref[np.float64][1])
    assert (M[..., :3] > 0).any()
    for which, (w, h) in ((oh.LUT_TRANSMITTANCE, dims[0:2]), (oh.LUT_MULTISCATTER, dims[2:4]), (oh.LUT_SKYVIEW, dims[4:6])):
        ptr, lw, lh = ctx.atmosphere_lut_ptr(which)
        assert ptr and ptr % 16 == 0 and (lw, lh) == (w, h)
    for sun in SUNS:
        ctx.sky_update(sun)
        S = ctx.atmosphere_lut(oh.LUT_SKYVIEW)
        assert S.shape == (dims[5], dims[4], 4)
        check_sky(dims, sun, S)
    ctx.close()


def test_default_tables_match_the_restatement():
    """AtmosphereController's own sizes and parameters, once: 64 x 256, 64 x 64 and 256 x 128."""
    dims, params, sun = oh.ATMOSPHERE_DEFAULT_DIMS, oh.atmosphere_params(), (0.3, 0.5, 0.4)
    ctx = oh.OceanContext(64, 1, 1)
    ctx.atmosphere()
    ctx.sky_update(sun)
    got = [ctx.atmosphere_lut(k) for k in range(3)]
    ctx.close()
    ref = reference_tm(dims, params.tobytes())
    check_table("transmittance", got[0], ref[f32][0], ref[np.float64][0])
    check_table("multiscatter", got[1], ref[f32][1], ref[np.float64][1])
    s32, s64, ends = reference_sky(dims, sun, params)
    rows = ends.any(axis=1)
    print(f"{int(rows.sum())} of {len(rows)} rows of the sky view end on the planet")
    assert 2 * rows.sum() <= len(rows)
    check_table("sky view", got[2], s32, s64, ~ends)
    assert np.isfinite(got[0]).all() and (got[0][..., :3] <= 1).all() and (got[0][..., :3] >= 0).all()


def test_same_call_twice_and_two_contexts_are_bit_identical():
    dims, sun = SMALL[1], SUNS[0]
    a, b = fresh(dims), fresh(dims)
    a.sky_update(sun)
    b.sky_update(sun)
    first = [a.atmosphere_lut(k) for k in range(3)]
    for k in range(3):
        np.testing.assert_array_equal(first[k], b.atmosphere_lut(k))
    a.atmosphere(PARAMS, dims)
    a.sky_update(sun)
    for k in range(3):
        np.testing.assert_array_equal(first[k], a.atmosphere_lut(k))
    # the defaults, where the multiscatter table is 4096 waves over many workgroups
    c, d = oh.OceanContext(64, 1, 1), oh.OceanContext(64, 1, 1)
    for ctx in (c, d):
        ctx.atmosphere()
        ctx.sky_update(sun)
    for k in range(3):
        np.testing.assert_array_equal(c.atmosphere_lut(k), d.atmosphere_lut(k))
    for ctx in (a, b, c, d):
        ctx.close()


def test_a_second_sun_equals_a_fresh_context():
    dims = SMALL[1]
    a = fresh(dims)
    a.sky_update(SUNS[0])
    first = a.atmosphere_lut(oh.LUT_SKYVIEW)
    a.sky_update(SUNS[1])
    second = a.atmosphere_lut(oh.LUT_SKYVIEW)
    b = fresh(dims)
    b.sky_update(SUNS[1])
    np.testing.assert_array_equal(second, b.atmosphere_lut(oh.LUT_SKYVIEW))
    assert not np.array_equal(first, second)
    # the unnormalised sun is its unit vector's table
    b.sky_update(SUNS[5])
    long = b.atmosphere_lut(oh.LUT_SKYVIEW)
    b.sky_update(tuple(A.normalise_sun(SUNS[5])))
    np.testing.assert_allclose(b.atmosphere_lut(oh.LUT_SKYVIEW), long, rtol=1e-4, atol=1e-7)
    # other sizes on the same context: the tables are reallocated
    a.atmosphere(PARAMS, SMALL[0])
    a.sky_update(SUNS[0])
    c = fresh(SMALL[0])
    c.sky_update(SUNS[0])
    for k in range(3):
        got = a.atmosphere_lut(k)
        assert got.shape == (SMALL[0][2 * k + 1], SMALL[0][2 * k], 4)
        np.testing.assert_array_equal(got, c.atmosphere_lut(k))
    for ctx in (a, b, c):
        ctx.close()


def test_state_refusals_and_kernel_kinds():
    ctx = oh.OceanContext(64, 1, 1)
    for call in (lambda: ctx.sky_update(SUNS[0]), lambda: ctx.sun_color(SUNS[0]), lambda: ctx.atmosphere_lut(0),
                 lambda: ctx.atmosphere_lut_ptr(2)):
        with pytest.raises(oh.OceanError) as e:
            call()
        assert e.value.code == oh.E_STATE and "ocean_atmosphere must precede" in str(e.value)
    out = np.zeros(4, f32)
    assert ctx.lib.ocean_atmosphere_read(ctx._h, 0, out.ctypes.data, 16) == oh.E_STATE
    ctx.set_kernel_timing(True)
    ctx.atmosphere(PARAMS, SMALL[0])
    assert "k_multiscatter" in ctx.kernel_name(2)
    for which in (oh.LUT_TRANSMITTANCE, oh.LUT_MULTISCATTER):
        assert ctx.atmosphere_lut(which).any()
    with pytest.raises(oh.OceanError) as e:
        ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    assert e.value.code == oh.E_STATE and "stale" in str(e.value)
    assert ctx.atmosphere_lut_ptr(oh.LUT_SKYVIEW)[1:] == (16, 8)  # the pointer itself is there
    ctx.sky_update(SUNS[0])
    assert "k_skyview" in ctx.kernel_name(2)
    ms, launches = ctx.kernel_stats(2)
    assert launches == 3 and ms > 0  # the three launches count as kind 2
    assert ctx.kernel_stats(0)[1] == 0 and ctx.kernel_stats(1)[1] == 0
    sky = ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    assert sky.shape == (8, 16, 4)
    buf = np.zeros(sky.size + 4, f32)
    for nbytes in (sky.nbytes - 16, sky.nbytes + 16, 0):
        assert ctx.lib.ocean_atmosphere_read(ctx._h, oh.LUT_SKYVIEW, buf.ctypes.data, nbytes) == oh.E_INVALID_ARG
        assert b"byte count" in ctx.lib.ocean_last_error()
    assert not buf.any()
    ctx.atmosphere(PARAMS, SMALL[0])  # the same sizes: stale again
    with pytest.raises(oh.OceanError) as e:
        ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    assert e.value.code == oh.E_STATE
    # a refused ocean_atmosphere leaves the context as it was: its tables stand, the sky view still stale
    with pytest.raises(oh.OceanError) as e:
        ctx.atmosphere(PARAMS, (8, 16, 8, 8, 16, 1))
    assert e.value.code == oh.E_INVALID_ARG and "skyview_height" in str(e.value)
    ctx.sky_update(SUNS[1])
    assert ctx.atmosphere_lut(oh.LUT_SKYVIEW).shape == (8, 16, 4)
    ctx.close()


@pytest.mark.parametrize("dims", [SMALL[1], SMALL[2], oh.ATMOSPHERE_DEFAULT_DIMS])
def test_sun_color_equals_the_restatement_over_the_device_column(dims):
    """The host arithmetic of ocean_sun_color is fp32 +, -, *, / alone: bit for bit the restatement over column 0 of the
    device's own transmittance table.  At the defaults the noon sun is the brightest and a sun below the horizon is
    black."""
    ctx = fresh(dims, oh.atmosphere_params())
    col = ctx.atmosphere_lut(oh.LUT_TRANSMITTANCE)[:, 0, :]
    suns = SUNS + [(0.0, -1.0, 0.0), (1.0, -0.98 * 2 + 1, 0.0), (0.2, 0.13, -0.4)]
    got = {}
    for sun in suns:
        got[sun] = ctx.sun_color(sun)
        assert got[sun].dtype == f32 and got[sun].shape == (3,)
        np.testing.assert_array_equal(got[sun], A.sun_color(col, sun, f32), err_msg=str(sun))
    ctx.atmosphere(oh.atmosphere_params(rayleigh_scale_height=4000.0), dims)  # the column is fetched again
    thin = ctx.sun_color(SUNS[0])
    np.testing.assert_array_equal(thin, A.sun_color(ctx.atmosphere_lut(oh.LUT_TRANSMITTANCE)[:, 0, :], SUNS[0], f32))
    if dims[1] >= 20:
        assert not np.array_equal(thin, got[SUNS[0]])
        assert (got[(0.0, 1.0, 0.0)] >= got[SUNS[1]]).all() and (got[(0.0, 1.0, 0.0)] > 0).all()
        assert not got[(0.0, -1.0, 0.0)].any()
    ctx.close()
