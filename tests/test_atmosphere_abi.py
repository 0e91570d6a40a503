"""CPU tests of the atmosphere (ocean_atmosphere, ocean_sky_update, ocean_atmosphere_read, ocean_atmosphere_lut,
ocean_sun_color and the camera's OCEAN_CAMERA_SKY_LUT mode; include/ocean/ocean.h): the symbols, constants and ctypes
signatures, every refusal that precedes the context test (reached with a null context, by the argument's name), and
the numpy restatement tests/atmosphere_ref.py pinned by answers known in closed form."""
import ctypes
import os

import numpy as np

import atmosphere_ref as A
import ocean_hip as oh

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("ocean_atmosphere", "ocean_sky_update", "ocean_atmosphere_read", "ocean_atmosphere_lut", "ocean_sun_color")
vp = ctypes.c_void_p


def test_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS and hasattr(L, s)
    assert (oh.ATMOSPHERE_FLOATS, oh.ATMOSPHERE_MAX_DIM, oh.CAMERA_SKY_LUT) == (32, 1024, 16)
    assert (oh.LUT_TRANSMITTANCE, oh.LUT_MULTISCATTER, oh.LUT_SKYVIEW) == (0, 1, 2)
    assert oh.ATMOSPHERE_DEFAULT_DIMS == (64, 256, 64, 64, 256, 128)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    for name, args in (("ocean_atmosphere", [P, P, i, i, i, i, i, i]), ("ocean_sky_update", [P, P]),
                       ("ocean_atmosphere_read", [P, i, P, sz]),
                       ("ocean_atmosphere_lut", [P, i, ctypes.POINTER(P), ctypes.POINTER(sz), ctypes.POINTER(sz)]),
                       ("ocean_sun_color", [P, P, P])):
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("atmosphere", "sky_update", "atmosphere_lut", "atmosphere_lut_ptr", "sun_color"):
        assert callable(getattr(oh.OceanContext, name)), name
    header = open(os.path.join(ROOT, "include", "ocean", "ocean.h")).read()
    for name, value in (("ATMOSPHERE_FLOATS", 32), ("ATMOSPHERE_MAX_DIM", 1024), ("LUT_TRANSMITTANCE", 0),
                        ("LUT_MULTISCATTER", 1), ("LUT_SKYVIEW", 2)):
        assert f"#define OCEAN_{name} {value}\n" in header, name
    assert "#define OCEAN_CAMERA_SKY_LUT 16 " in header


def test_atmosphere_params_fields_and_defaults():
    """AtmosphereController.cs:21-36 and Atmosphere.shader:4."""
    p = oh.atmosphere_params()
    assert p.dtype == f32 and p.shape == (32,)
    want = [6360000, 6420000, 5.802e-6, 13.558e-6, 6.5e-5, 0, 0, 0, 8000, 3.996e-6, 3.996e-6, 3.996e-6, 4.4e-6, 4.4e-6,
            4.4e-6, 1200, 0.85, 0, 0, 0, 0.65e-6, 1.881e-6, 0.085e-6, 0, 0, 0, 0.04, 0, 0, 0, 0, 0]
    np.testing.assert_array_equal(p, np.float64(want).astype(f32))
    q = oh.atmosphere_params(planet_radius=1.0, atmosphere_radius=2.0, rayleigh_scattering=(3, 4, 5),
                             rayleigh_absorption=(6, 7, 8), rayleigh_scale_height=9, mie_scattering=(10, 11, 12),
                             mie_absorption=(13, 14, 15), mie_scale_height=16, g=17, ozone_scattering=(18, 19, 20),
                             ozone_absorption=(21, 22, 23), ground_albedo=(24, 25, 26), sun_size=27)
    np.testing.assert_array_equal(q, np.r_[np.arange(1, 28), np.zeros(5)].astype(f32))


# ---------------------------------------------------------------------------- the refusals
def _message(L):
    return L.ocean_last_error().decode()


def _atmosphere(L, params=None, dims=(0,) * 6, null=False):
    p = np.ascontiguousarray(oh.atmosphere_params() if params is None else params, f32)
    L.ocean_host_alloc(0, None)  # (leaves another message behind)
    rc = L.ocean_atmosphere(None, None if null else vp(p.ctypes.data), *dims)
    return rc, _message(L)


def _with(index, value):
    p = oh.atmosphere_params()
    p[index] = value
    return p


def test_ocean_atmosphere_refuses_by_argument_name_before_the_context():
    L = oh.load_library()
    bad = [(dict(null=True), "null params"), (dict(params=_with(3, np.nan)), "params[3]"),
           (dict(params=_with(26, np.inf)), "params[26]"), (dict(params=_with(31, -np.inf)), "params[31]"),
           (dict(params=_with(0, 0.0)), "planetRadius"), (dict(params=_with(0, -6360000.0)), "planetRadius"),
           (dict(params=_with(1, 6360000.0)), "atmosphereRadius"), (dict(params=_with(1, 100.0)), "atmosphereRadius"),
           (dict(params=_with(8, 0.0)), "scale height"), (dict(params=_with(15, -1200.0)), "scale height"),
           (dict(params=_with(27, 1.0)), "params[27] is reserved"), (dict(params=_with(31, -0.5)), "params[31] is reserved")]
    names = ("transmittance_width", "transmittance_height", "multiscatter_width", "multiscatter_height", "skyview_width",
             "skyview_height")
    for k, name in enumerate(names):
        for v in (1, 0, -4, 1025):
            d = list(oh.ATMOSPHERE_DEFAULT_DIMS)
            d[k] = v
            bad.append((dict(dims=tuple(d)), name))
    for kw, word in bad:
        rc, msg = _atmosphere(L, **kw)
        assert rc == oh.E_INVALID_ARG and word in msg, (kw, msg)
    # valid arguments reach the context test: the defaults, explicit sizes and the limits themselves
    for dims in ((0,) * 6, oh.ATMOSPHERE_DEFAULT_DIMS, (2,) * 6, (1024,) * 6, (12, 20, 3, 5, 20, 12)):
        rc, msg = _atmosphere(L, dims=dims)
        assert rc == oh.E_INVALID_ARG and "context" in msg, (dims, msg)


def test_sun_which_and_null_pointers_are_refused_before_the_context():
    L = oh.load_library()
    rgb, out = np.zeros(3, f32), np.zeros(16, f32)
    suns = [(None, "null sun"), ((0, 0, 0), "length"), ((np.nan, 1, 0), "sun[0]"), ((0, 1, np.inf), "sun[2]"),
            ((0, -np.inf, 0), "sun[1]"), ((3e38, 3e38, 3e38), "length"), ((1e-30, 0, 1e-30), "length")]
    for sun, word in suns:
        s = None if sun is None else np.asarray(sun, f32)
        ptr = None if s is None else vp(s.ctypes.data)
        assert L.ocean_sky_update(None, ptr) == oh.E_INVALID_ARG and word in _message(L), sun
        assert L.ocean_sun_color(None, ptr, vp(rgb.ctypes.data)) == oh.E_INVALID_ARG and word in _message(L), sun
    s = np.asarray((0.3, 0.5, 0.4), f32)
    assert L.ocean_sun_color(None, vp(s.ctypes.data), None) == oh.E_INVALID_ARG and "null rgb" in _message(L)
    assert L.ocean_sky_update(None, vp(s.ctypes.data)) == oh.E_INVALID_ARG and "context" in _message(L)
    assert L.ocean_sun_color(None, vp(s.ctypes.data), vp(rgb.ctypes.data)) == oh.E_INVALID_ARG and "context" in _message(L)
    assert not rgb.any()
    dev, w, h = ctypes.c_void_p(), ctypes.c_size_t(), ctypes.c_size_t()
    for which in (-1, 3, 16):
        assert L.ocean_atmosphere_read(None, which, vp(out.ctypes.data), 64) == oh.E_INVALID_ARG and "which" in _message(L)
        assert L.ocean_atmosphere_lut(None, which, ctypes.byref(dev), ctypes.byref(w), ctypes.byref(h)) == oh.E_INVALID_ARG
        assert "which" in _message(L)
    assert L.ocean_atmosphere_read(None, 0, None, 64) == oh.E_INVALID_ARG and "null output" in _message(L)
    for args in ((None, ctypes.byref(w), ctypes.byref(h)), (ctypes.byref(dev), None, ctypes.byref(h)),
                 (ctypes.byref(dev), ctypes.byref(w), None)):
        assert L.ocean_atmosphere_lut(None, 0, *args) == oh.E_INVALID_ARG and "null dev, width or height" in _message(L)
    for which in (0, 1, 2):
        assert L.ocean_atmosphere_read(None, which, vp(out.ctypes.data), 64) == oh.E_INVALID_ARG and "context" in _message(L)
        assert L.ocean_atmosphere_lut(None, which, ctypes.byref(dev), ctypes.byref(w), ctypes.byref(h)) == oh.E_INVALID_ARG
        assert "context" in _message(L)
    assert not out.any()


def _camera(L, name, mode, material=True, nbytes=None):
    cam = oh.look_at_camera((0, 10, 0), (0, 0, 30), (0, 1, 0), 0.8, 4, 3, 0, 90)
    mat = oh.material() if material is True else material
    out = np.zeros(4 * 3 * 8, f32)
    req = ctypes.c_void_p(0x1234)
    args = [None, 0, mode, 2, 16, 4, vp(cam.ctypes.data), None if mat is None else vp(mat.ctypes.data), 4, 3,
            vp(out.ctypes.data), 4 * 3 * 16 if nbytes is None else nbytes]
    rc = getattr(L, name)(*args, *((ctypes.byref(req),) if name.endswith("_async") else ()))
    assert not out.any() and (not name.endswith("_async") or req.value is None)
    return rc, _message(L)


def test_camera_sky_mode_values():
    """The flag is valid only with OCEAN_CAMERA_COLOR; mode 3 stays invalid; bytes and material as in colour mode."""
    L = oh.load_library()
    sky = oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT
    for name in ("ocean_camera", "ocean_camera_device", "ocean_camera_async"):
        for mode in (oh.CAMERA_HITS | oh.CAMERA_SKY_LUT, oh.CAMERA_RANGE | oh.CAMERA_SKY_LUT, 3, 19, oh.CAMERA_SKY_LUT * 2,
                     sky | 4):
            rc, msg = _camera(L, name, mode)
            assert rc == oh.E_INVALID_ARG and "mode" in msg, (name, mode, msg)
        rc, msg = _camera(L, name, sky, material=None)
        assert rc == oh.E_INVALID_ARG and "material" in msg
        rc, msg = _camera(L, name, sky, material=np.r_[np.zeros(28), np.nan, np.zeros(3)].astype(f32))
        assert rc == oh.E_INVALID_ARG and "material[28]" in msg  # ignored by the mode, still refused
        for nbytes in (4 * 3 * 32, 4 * 3 * 4, 0):
            rc, msg = _camera(L, name, sky, nbytes=nbytes)
            assert rc == oh.E_INVALID_ARG and "byte count" in msg
        rc, msg = _camera(L, name, sky)
        assert rc == oh.E_INVALID_ARG and "context" in msg, (name, msg)


# ---------------------------------------------------------------------------- the restatement, by known answers
def test_zenith_ray_from_the_ground_has_the_closed_form_rayleigh_depth():
    """Rayleigh alone: the optical depth along the zenith ray from the ground is the integral of beta e^(-h / H) over
    the 60 km, beta H (1 - e^(-60000 / 8000)).  The march is the midpoint rule with 500 steps of dh = 120 m, whose own
    error is at most (60000 / 24) dh^2 max |f''| = (60000 / 24) 120^2 beta / H^2 = 0.5625 beta, 7e-5 of the depth."""
    beta = np.float64(f32([5.802e-6, 13.558e-6, 6.5e-5]))
    p = oh.atmosphere_params(mie_scattering=(0, 0, 0), mie_absorption=(0, 0, 0), ozone_absorption=(0, 0, 0))
    P = A.Params(p, np.float64)
    tau = -np.log(A.transmittance_at(P, P.Rp, 1.0))
    exact = beta * 8000.0 * (1.0 - np.exp(-60000.0 / 8000.0))
    rule = (60000.0 / 24.0) * 120.0 ** 2 * beta / 8000.0 ** 2
    assert tau.shape == (3,) and (np.abs(tau - exact) <= rule * (1 + 1e-6)).all(), (tau, exact, rule)
    assert (np.abs(tau - exact) > 0.05 * rule).all()  # and it is the rule's error that is seen, not a looser match
    t32 = -np.log(A.transmittance_at(A.Params(p, f32), f32(P.Rp), f32(1)).astype(np.float64))
    np.testing.assert_allclose(t32, exact, rtol=2e-4)


def test_transmittance_is_one_at_the_top_looking_up_and_zero_through_the_planet():
    p = oh.atmosphere_params()
    for t in (f32, np.float64):
        P = A.Params(p, t)
        np.testing.assert_array_equal(A.transmittance_at(P, P.Ra, t(1)), np.ones(3, t))
        np.testing.assert_array_equal(A.transmittance_at(P, P.Rp, t(-1)), np.zeros(3, t))
    T = A.transmittance(p, 8, 16, f32)
    assert T.dtype == f32 and T.shape == (16, 8, 4) and np.isfinite(T).all() and not T[..., 3].any()
    assert ((T[..., :3] >= 0) & (T[..., :3] <= 1)).all()
    assert (np.diff(T[12:, :, :3], axis=1) >= 0).all()  # looking up: less air above a higher start


def test_multiscatter_of_a_non_scattering_atmosphere_is_zero():
    p = oh.atmosphere_params(rayleigh_scattering=(0, 0, 0), rayleigh_absorption=(5.8e-6, 1.35e-5, 3.3e-5),
                             mie_scattering=(0, 0, 0))
    for t in (f32, np.float64):
        T = A.transmittance(p, 8, 16, t)
        M = A.multiscatter(p, T, 5, 3, t)
        assert M.dtype == t and M.shape == (3, 5, 4)
        np.testing.assert_array_equal(M[..., :3], 0)
        np.testing.assert_array_equal(M[..., 3], 1)
    # and a scattering one is not: positive where the sun is up
    p = oh.atmosphere_params()
    M = A.multiscatter(p, A.transmittance(p, 8, 16, f32), 5, 4, f32)
    assert np.isfinite(M).all() and (M[2:, :, :3] > 0).all()


def test_butterfly_is_the_fold_of_the_halves():
    a = np.random.default_rng(1).normal(size=(2, 64, 3)).astype(f32)
    lanes = a.copy()
    for s in (32, 16, 8, 4, 2, 1):  # a_i = a_i + a_(i xor s), every lane
        lanes = lanes + lanes[:, np.arange(64) ^ s, :]
    np.testing.assert_array_equal(A.butterfly(a), lanes[:, 0, :])
    assert A.butterfly(a).dtype == f32


def test_lut_read_taps_and_clamps():
    L = np.zeros((3, 4, 4), f32)
    L[..., 0] = np.arange(4, dtype=f32)[None, :]
    L[..., 1] = np.arange(3, dtype=f32)[:, None]
    centres_u, centres_v = (np.arange(4) + 0.5) / 4, (np.arange(3) + 0.5) / 3
    for i, u in enumerate(centres_u):
        for j, v in enumerate(centres_v):
            np.testing.assert_allclose(A.lut_read(L, f32(u), f32(v), f32)[:2], [i, j], atol=1e-6)
    np.testing.assert_array_equal(A.lut_read(L, f32(-3), f32(7), f32)[:2], [0, 2])   # clamped
    np.testing.assert_array_equal(A.lut_read(L, f32(np.nan), f32(0), f32)[:2], [0, 0])
    np.testing.assert_allclose(A.lut_read(L, f32(0.5), f32(0.5), np.float64)[:2], [1.5, 1.0], atol=1e-12)


def test_sun_color_gradient_hits_its_keys():
    """Over the ramp column (y, 2 y, 3 y) a bilinear read at t is Y = t H - 0.5 itself, so key_k = 2.5 (t_k H - 0.5)
    (1, 2, 3).  A sun at the elevation e = t_k returns key_k, one half-way between two keys their mean, and suns
    beyond the first and last key those keys."""
    H = 256
    col = np.arange(H, dtype=np.float64)[:, None] * np.array([1.0, 2.0, 3.0])[None, :]
    keys = [2.5 * (np.float64(f32(t)) * H - 0.5) * np.array([1.0, 2.0, 3.0]) for t in A.SUN_KEYS]

    def sun_at(e):
        y = 2.0 * e - 1.0
        return (np.sqrt(1.0 - y * y), y, 0.0)

    for t in (f32, np.float64):
        tol = 2e-3 if t is f32 else 2e-4  # e comes from an fp32 unit vector: 1e-7 of 2.5 H (1, 2, 3) per unit of e
        for k, tk in enumerate(A.SUN_KEYS):
            got = A.sun_color(col, sun_at(tk), t)
            assert got.dtype == t
            np.testing.assert_allclose(got, keys[k], atol=tol)
        for k in range(7):
            mid = 0.5 * (A.SUN_KEYS[k] + A.SUN_KEYS[k + 1])
            np.testing.assert_allclose(A.sun_color(col, sun_at(mid), t), 0.5 * (keys[k] + keys[k + 1]), atol=tol)
        np.testing.assert_allclose(A.sun_color(col, (0, -1, 0), t), keys[0], rtol=1e-6)
        np.testing.assert_allclose(A.sun_color(col, (0, 5, 0), t), keys[7], rtol=1e-6)
        np.testing.assert_allclose(A.sun_color(col, (0.05, -1, 0.05), t), keys[0], rtol=1e-6)


def test_sky_lookup_maps_directions_to_the_table():
    """SKY(r) over a table whose channels are the texel's column and row: the zenith reads the last row, the horizon
    and everything below it the middle, azimuth 0 (+z) the middle column, and the length of r does not matter."""
    W, H = 16, 8
    S = np.zeros((H, W, 4), np.float64)
    S[..., 0] = np.arange(W)[None, :]
    S[..., 1] = np.arange(H)[:, None]
    r = np.array([[0, 1, 0], [0, 0, 1], [0, -0.7, 1], [0, 0, 5], [1, 0, 0], [-1, 0, 0], [0, 3, 0]], np.float64)
    got = A.sky_lookup(S, r, np.float64) / 2
    np.testing.assert_allclose(got[[0, 6], 1], H - 1)
    np.testing.assert_allclose(got[[1, 2, 3, 4, 5], 1], 0.5 * H - 0.5, atol=1e-6)
    np.testing.assert_allclose(got[[1, 2, 3], 0], 0.5 * W - 0.5, atol=1e-5)
    np.testing.assert_allclose(got[4, 0], 0.75 * W - 0.5, atol=1e-5)
    np.testing.assert_allclose(got[5, 0], 0.25 * W - 0.5, atol=1e-5)
    a32 = A.sky_lookup(S, r, f32)
    assert a32.dtype == f32
    np.testing.assert_allclose(a32, 2 * got[:, :3], atol=1e-4)


def test_sun_spot_is_one_at_the_sun_and_zero_outside_the_disc_and_below_the_horizon():
    light = np.float64([0.3, 0.5, 0.4])
    light /= np.linalg.norm(light)
    m = oh.material(light_direction=light)
    d = np.array([m[20:23], [0.0, 1.0, 0.0], [light[0], -light[1], light[2]]], np.float64)
    np.testing.assert_allclose(A.sun_spot(d, m, 0.04, np.float64), [1, 0, 0], atol=1e-9)
    near = np.float64(m[20:23]) + np.array([0.02, 0, 0])
    s = A.sun_spot((near / np.linalg.norm(near))[None, :], m, 0.04, np.float64)[0]
    assert 0.2 < s < 0.8  # half-way across the disc's edge: 1 - smoothstep(0.5)
