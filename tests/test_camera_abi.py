"""CPU tests of the camera views (ocean_camera, _device, _async; include/ocean/ocean.h): what can be checked without
a GPU -- the symbols, the constants, the ctypes signatures, the validation that precedes every device call (all of
it but the tile and the slot size needs no context, so it is reached with a null one), the helpers that build a
camera and a material, and restate_camera, the numpy fp32 statement of an image that tests/test_gpu_camera.py
compares the kernel with.  The restatement is built on restate_raycast (tests/test_ray_abi.py); its shading,
shade(), is written once over a dtype, so the same statements give the fp32 restatement and the float64 evaluation
that measures its rounding.  Here it runs on a flat sea, where range and colour are known in closed form."""
import ctypes
import os

import numpy as np

import ocean_hip as oh
import oracle as O
from test_gpu_query import restate_surface
from test_ray_abi import _oracle_textures, ray_positions, restate_raycast

f32 = np.float32
CAMERA_SYMBOLS = ("ocean_camera", "ocean_camera_device", "ocean_camera_async")
PIXEL_FLOATS = {oh.CAMERA_HITS: 8, oh.CAMERA_RANGE: 1, oh.CAMERA_COLOR: 4}
PI32, TINY32 = f32(3.14159265358979), f32(1.175494351e-38)


# ---------------------------------------------------------------------------- the restatement
def camera_rays(camera, w, h):
    """The rays of ocean.h's pixels, [h * w][8], pixel (i, j) at row j * w + i: fp32, one rounding per operation."""
    c = np.ascontiguousarray(camera, f32)
    o, d00, du, dv = c[0:3], c[3:6], c[6:9], c[9:12]
    fi = np.tile(np.arange(w, dtype=f32), h)[:, None]
    fj = np.repeat(np.arange(h, dtype=f32), w)[:, None]
    raw = (d00[None, :] + fi * du[None, :]) + fj * dv[None, :]
    ln = np.sqrt((raw[:, 0] * raw[:, 0] + raw[:, 1] * raw[:, 1]) + raw[:, 2] * raw[:, 2])
    rays = np.empty((w * h, 8), f32)
    rays[:, 0:3] = o
    rays[:, 3:6] = raw / ln[:, None]
    rays[:, 6], rays[:, 7] = c[12], c[13]
    assert raw.dtype == f32 and ln.dtype == f32
    return rays


def sample_at(tex, p, lod):
    """ocean_sample_world at (p.x, p.z, lod) over `tex`: its mip chains where it has them (tex.deriv_mips)."""
    pts = np.concatenate([p, np.asarray(lod, f32)[:, None]], axis=1).astype(f32)
    return O.sample_world(tex.disp, tex.deriv, tex.turb, tex.lengths, pts, getattr(tex, "deriv_mips", None),
                          getattr(tex, "turb_mips", None))


def shade(d, n, eta, foam, material, has_foam, dtype=f32):
    """ocean.h's colour of a hit pixel, statement by statement, in `dtype`: d, n [M][3], eta, foam [M] -> [M][3]."""
    t = dtype
    d, n, eta, foam = (np.asarray(a).astype(t) for a in (d, n, eta, foam))
    m = np.asarray(material, f32).astype(t)
    pi, tiny, one, zero = t(PI32), t(TINY32), t(1), t(0)
    C, r0, fe, fd, rho, ex, ey, ke, ks = m[0:3], m[3], m[4], m[5], m[6], m[8], m[9], m[10], m[11]
    ss, ft, fc, fb, L, lc, hz, zn = m[12:15], m[15], m[16:19], m[19], m[20:23], m[23:26], m[26:29], m[29:32]

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def sat(x):
        return np.minimum(np.maximum(x, zero), one)

    V = -d
    hr = V + L[None, :]
    h = hr / np.sqrt(dot(hr, hr))[:, None]
    ndv, ndl, hdv, hdn = dot(n, V), dot(n, L[None, :]), dot(h, V), dot(h, n)
    F = r0 + ((one - r0) * np.power(one - sat(ndv), fe)) / fd
    x = one - sat(hdv)
    FH = r0 + (one - r0) * (((x * x) * (x * x)) * x)
    s = np.maximum(zero, dot(L[None, :], d))
    g = np.maximum(zero, eta) * ((s * s) * (s * s))
    ry = (t(2) * ndv) * n[:, 1] - V[:, 1]
    sky = hz[None, :] + sat(ry)[:, None] * (zn - hz)[None, :]
    env = (sky * pi) * ke
    refraction = C[None, :] + (g[:, None] * ss[None, :]) * lc[None, :]
    if L[1] > 0:
        den = np.maximum(one - h[:, 2] * h[:, 2], tiny)
        c2, s2 = np.maximum((h[:, 0] * h[:, 0]) / den, zero), np.maximum((h[:, 1] * h[:, 1]) / den, zero)
        nu, nv = (ex * t(10)) * (one - rho), (ey * t(10)) * (one - rho)
        D = np.sqrt((nu + one) * (nv + one)) * np.power(np.maximum(hdn, zero), nu * c2 + nv * s2)
        A = np.maximum((D * FH) / np.maximum(((t(8) * pi) * hdv) * np.maximum(ndv, ndl), tiny), zero)
        ash = lc[None, :] * A[:, None]
        a2 = (rho * rho) * (rho * rho)
        q = (sat(hdn) * sat(hdn)) * (a2 - one) + one
        N = np.maximum(a2 / np.maximum(pi * (q * q), tiny), zero)
        k = rho / t(2)
        G = np.maximum((sat(ndv) / np.maximum(sat(ndv) * (one - k) + k, tiny)) *
                       (sat(ndl) / np.maximum(sat(ndl) * (one - k) + k, tiny)), zero)
        cook = ((lc[None, :] * N[:, None]) * G[:, None]) / np.maximum((t(8) * sat(ndv)) * sat(ndl), tiny)[:, None]
    else:
        ash = cook = np.zeros((len(d), 3), t)
    reflections = env + (cook + ash * sat(ndv)[:, None]) * ks
    e = refraction + F[:, None] * (reflections - refraction)
    if has_foam:
        foamy = foam >= ft
        e = np.where(foamy[:, None], e + fb * (fc[None, :] - e), e)
    assert e.dtype == t
    return e


def shading_inputs(tex, camera, material, w, h, k, steps, refine):
    """What the colour of every pixel is formed from, all fp32: the rays, their ocean_raycast records, and at the
    hit pixels the normal, the wave height and the foam of the sample at p_K with the pixel's lod."""
    rays = camera_rays(camera, w, h)
    rec = restate_raycast(tex, rays, k, steps, refine)
    hit = np.flatnonzero(rec[:, 3] == oh.RAY_HIT)
    q = ray_positions(rays[hit], rec[hit, 0])
    pk = restate_surface(tex, np.ascontiguousarray(q[:, [0, 2]]), (k,))[k][:, 1:3]
    lod = rec[hit, 0] * f32(np.asarray(material, f32)[7])
    s = sample_at(tex, pk, lod)
    return rays, rec, hit, s[:, 2, :3], s[:, 0, 1], s[:, 0, 3]


def colours(rays, rec, hit, n, eta, foam, material, has_foam, dtype=f32):
    """The colour image [M][4] from shading_inputs' arrays: shade() at the hits, the sky after a miss, the water
    colour under water, each in `dtype`; the status in channel 3."""
    m = np.asarray(material, f32).astype(dtype)
    out = np.empty((len(rays), 4), dtype)
    dy = rays[:, 4].astype(dtype)
    sat = np.minimum(np.maximum(dy, dtype(0)), dtype(1))
    out[:, :3] = m[26:29][None, :] + sat[:, None] * (m[29:32] - m[26:29])[None, :]
    out[rec[:, 3] == oh.RAY_SUBMERGED, :3] = m[0:3]
    out[hit, :3] = shade(rays[hit, 3:6], n, eta, foam, material, has_foam, dtype)
    out[:, 3] = rec[:, 3]
    return out


def restate_camera(tex, camera, material, w, h, mode, k, steps, refine):
    """ocean.h's definition of ocean_camera in numpy fp32, operation by operation: [h * w][8], [h * w] or [h * w][4]."""
    if mode != oh.CAMERA_COLOR:
        rec = restate_raycast(tex, camera_rays(camera, w, h), k, steps, refine)
        if mode == oh.CAMERA_HITS:
            return rec
        return np.where(rec[:, 3] == oh.RAY_MISS, f32(np.inf), rec[:, 0]).astype(f32)
    args = shading_inputs(tex, camera, material, w, h, k, steps, refine)
    return colours(*args, material, tex.deriv is not None, f32)


# ---------------------------------------------------------------------------- the ABI
def test_camera_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in CAMERA_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.CAMERA_HITS, oh.CAMERA_RANGE, oh.CAMERA_COLOR) == (0, 1, 2)
    assert (oh.CAMERA_FLOATS, oh.CAMERA_MATERIAL_FLOATS) == (14, 32)
    assert (oh.CAMERA_MAX_PIXELS, oh.CAMERA_MAX_SAMPLES) == (1 << 22, 1 << 28)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    cam = [P, i, i, i, i, i, P, P, i, i, P, sz]
    for name, args in (("ocean_camera", cam), ("ocean_camera_device", cam),
                       ("ocean_camera_async", cam + [ctypes.POINTER(P)])):
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("camera", "camera_async", "camera_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.Camera) and callable(oh.look_at_camera) and callable(oh.material)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ocean", "ocean.h")).read()
    for name, value in (("HITS", 0), ("RANGE", 1), ("COLOR", 2), ("FLOATS", 14), ("MATERIAL_FLOATS", 32),
                        ("MAX_PIXELS", "(1 << 22)"), ("MAX_SAMPLES", "(1 << 28)")):
        assert f"#define OCEAN_CAMERA_{name} {value}\n" in header, name


def _call(L, name, kw):
    """One entry with the arguments `kw` over a valid base; (code, message, req after the call or "no req")."""
    cam = np.ascontiguousarray(kw.get("camera", oh.look_at_camera((0, 10, 0), (0, 0, 30), (0, 1, 0), 0.8, 4, 3, 0, 90)))
    mat = kw.get("material", oh.material())
    w, h, mode = kw.get("width", 4), kw.get("height", 3), kw.get("mode", oh.CAMERA_COLOR)
    nbytes = kw.get("bytes", w * h * 4 * PIXEL_FLOATS.get(mode, 0))
    out = np.zeros(4 * 3 * 8, f32)
    vp = ctypes.c_void_p
    args = [None, kw.get("tile", 0), mode, kw.get("iterations", 2), kw.get("steps", 16), kw.get("refine", 4),
            None if kw.get("null_camera") else vp(cam.ctypes.data), None if mat is None else vp(mat.ctypes.data), w, h,
            None if kw.get("null_out") else vp(out.ctypes.data + kw.get("misalign", 0)), nbytes]
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)  # (leaves another message behind)
    rc = getattr(L, name)(*args, *((ctypes.byref(req),) if name.endswith("_async") else ()))
    assert not out.any()
    return rc, L.ocean_last_error().decode(), req.value if name.endswith("_async") else "no req"


BAD = [(dict(null_camera=True), "null camera"), (dict(null_out=True), "null camera or output"),
       (dict(material=None), "material"), (dict(mode=3), "mode"), (dict(mode=-1), "mode"),
       (dict(iterations=-1), "iterations"), (dict(iterations=17), "iterations"), (dict(steps=0), "steps"),
       (dict(steps=oh.RAY_MAX_STEPS + 1), "steps"), (dict(refine=-1), "refine"), (dict(refine=33), "refine"),
       (dict(camera=np.r_[np.zeros(13), np.inf].astype(f32)), "camera[13]"),
       (dict(camera=np.r_[np.nan, np.ones(13)].astype(f32)), "camera[0]"),
       (dict(material=np.r_[np.zeros(31), -np.inf].astype(f32)), "material[31]"),
       (dict(material=np.r_[np.zeros(7), np.nan, np.zeros(24)].astype(f32), mode=oh.CAMERA_RANGE), "material[7]"),
       (dict(width=0), "width"), (dict(height=0), "height"), (dict(width=-5), "width"),
       (dict(width=1 << 11, height=(1 << 11) + 1, steps=1), "OCEAN_CAMERA_MAX_PIXELS"),
       (dict(width=1 << 16, height=1 << 16, steps=1), "OCEAN_CAMERA_MAX_PIXELS"),     # 2^32 pixels: 64-bit product
       (dict(width=1 << 11, height=1 << 11, steps=65), "OCEAN_CAMERA_MAX_SAMPLES"),   # 2^22 x 65 > 2^28
       (dict(width=1 << 11, height=1 << 11, steps=1024), "OCEAN_CAMERA_MAX_SAMPLES"),  # 2^32 samples
       (dict(bytes=4 * 3 * 16 - 4), "byte count"), (dict(mode=oh.CAMERA_RANGE, bytes=4 * 3 * 16), "byte count"),
       (dict(mode=oh.CAMERA_HITS, bytes=4 * 3 * 16), "byte count"), (dict(bytes=0), "byte count")]


def test_camera_validation_precedes_every_device_call():
    """No GPU here: each case returns OCEAN_E_INVALID_ARG with the argument's name, in all three forms, and *req is
    NULL afterwards.  Valid arguments reach the context test, which refuses the null context."""
    L = oh.load_library()
    for name in CAMERA_SYMBOLS:
        for kw, word in BAD:
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and word in msg, (name, kw, msg)
            assert req in (None, "no req"), (name, kw)
        for kw in (dict(), dict(mode=oh.CAMERA_HITS, material=None), dict(mode=oh.CAMERA_RANGE, material=None),
                   dict(width=1 << 11, height=1 << 11, steps=64, bytes=(1 << 22) * 16)):  # the limits themselves
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and "context" in msg, (name, kw, msg)
            assert req in (None, "no req")
    rc, msg, _ = _call(L, "ocean_camera_device", dict(misalign=4))
    assert rc == oh.E_INVALID_ARG and "aligned" in msg
    rc, msg, _ = _call(L, "ocean_camera", dict(misalign=4))  # a host buffer needs no alignment
    assert "context" in msg
    cam, out = np.zeros(14, f32), np.zeros(16, f32)
    assert L.ocean_camera_async(None, 0, oh.CAMERA_RANGE, 0, 1, 0, cam.ctypes.data, None, 2, 2, out.ctypes.data, 16,
                                None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


# ---------------------------------------------------------------------------- the helpers
def test_look_at_camera_gives_unit_central_rays_and_the_field_of_view():
    eye, target, fov, w, h = (3.0, 12.0, -7.0), (40.0, 2.0, 25.0), 0.9, 64, 48
    cam = oh.look_at_camera(eye, target, (0, 1, 0), fov, w, h, 0.5, 300.0)
    assert cam.dtype == f32 and cam.shape == (14,)
    np.testing.assert_array_equal(cam[[0, 1, 2, 12, 13]], f32([3, 12, -7, 0.5, 300]))
    c = cam.astype(np.float64)
    d00, du, dv = c[3:6], c[6:9], c[9:12]
    fwd = np.float64(target) - np.float64(eye)
    fwd /= np.linalg.norm(fwd)
    centre = d00 + du * (w - 1) / 2 + dv * (h - 1) / 2  # between the four central pixels
    np.testing.assert_allclose(centre, fwd, atol=1e-6)  # unit, along the view
    assert abs(du @ dv) < 1e-9 and abs(du @ fwd) < 1e-8 and abs(dv @ fwd) < 1e-8
    np.testing.assert_allclose(np.linalg.norm(du), np.linalg.norm(dv), rtol=1e-6)  # square pixels
    top, bottom = centre - dv * h / 2, centre + dv * h / 2  # the image's upper and lower edge
    angle = np.arccos(top @ bottom / np.linalg.norm(top) / np.linalg.norm(bottom))
    np.testing.assert_allclose(angle, fov, rtol=1e-6)
    assert dv[1] < 0 and np.cross(fwd, [0, 1, 0]) @ du > 0  # row 0 is the top, column 0 the left
    rays = camera_rays(cam, w, h)
    np.testing.assert_allclose(np.linalg.norm(rays[:, 3:6].astype(np.float64), axis=1), 1.0, atol=2e-7)
    mid = rays[(h // 2) * w + w // 2, 3:6]
    assert np.arccos(np.clip(mid.astype(np.float64) @ fwd, -1, 1)) < 1.5 * fov / h


def test_material_fields():
    m = oh.material(color=(0.1, 0.2, 0.3), roughness=0.3, ex=0.2, ey=0.4, environment_strength=0.7, sun_strength=0.9,
                    subsurface_intensity=0.5, subsurface_color=(0.2, 0.4, 0.6), foam_color=(0.9, 0.8, 0.7),
                    foam_threshold=1.25, foam_blending=0.6, light_direction=(3, 4, 0), light_color=(1, 0.9, 0.8),
                    horizon_color=(0.5, 0.6, 0.7), zenith_color=(0.1, 0.2, 0.9), lod_slope=0.01)
    assert m.dtype == f32 and m.shape == (32,)
    want = [0.1, 0.2, 0.3, (0.333 / 2.333) ** 2, 5 * np.exp(-2.69 * 0.3), 1 + 22.7 * 0.3 ** 1.5, 0.3, 0.01, 0.2, 0.4, 0.7,
            0.9, 0.1, 0.2, 0.3, 1.25, 0.9, 0.8, 0.7, 0.6, 0.6, 0.8, 0.0, 1, 0.9, 0.8, 0.5, 0.6, 0.7, 0.1, 0.2, 0.9]
    np.testing.assert_array_equal(m, np.float64(want).astype(f32))  # float64, rounded once


# ---------------------------------------------------------------------------- a flat sea
def _flat():
    n, cas = 32, O.SCENE_CASCADES[:2]
    tex = _oracle_textures(n, cas, np.zeros((n, n, 2), f32))
    assert not tex.disp[..., :3].any() and not tex.deriv.any()
    return tex


def test_flat_sea_range_and_colour_in_closed_form():
    """Zero noise: the water is the plane y = 0 with the normal (0, 1, 0).  From the height o.y a pixel whose ray
    descends meets it at t = o.y / -d.y; the march brackets that within dt and B bisections within dt / 2^B, and
    t* is the bracket's upper end.  Pixels that look above the horizon miss; from below the surface all are
    submerged.  The colour of a hit is the formula at n = (0, 1, 0), eta = 0: evaluated here in float64, and for a
    material without sun, subsurface term or foam in its closed form C + F (pi sky - C)."""
    tex = _flat()
    w, h, k, steps, refine = 9, 7, 2, 32, 6
    cam = oh.look_at_camera((1.5, 10.0, -2.0), (20.0, 6.0, 30.0), (0, 1, 0), 0.9, w, h, 0.0, 160.0)
    rays = camera_rays(cam, w, h)
    rng = restate_camera(tex, cam, None, w, h, oh.CAMERA_RANGE, k, steps, refine)
    hits = restate_camera(tex, cam, None, w, h, oh.CAMERA_HITS, k, steps, refine)
    dy = rays[:, 4].astype(np.float64)
    exact = np.where(dy < 0, 10.0 / -np.where(dy < 0, dy, -1.0), np.inf)
    hit = exact < 160.0
    assert 0.2 * w * h <= hit.sum() <= 0.9 * w * h
    np.testing.assert_array_equal(hits[:, 3], np.where(hit, oh.RAY_HIT, oh.RAY_MISS))
    np.testing.assert_array_equal(np.isinf(rng), ~hit)
    dt = 160.0 / steps
    err = rng[hit].astype(np.float64) - exact[hit]
    assert (err >= -1e-4).all() and (err <= dt / 2 ** refine + 1e-4).all(), (err.min(), err.max())
    np.testing.assert_array_equal(rng[hit], hits[hit, 0])
    np.testing.assert_array_equal(hits[hit, 4:7], np.tile(f32([0, 1, 0]), (hit.sum(), 1)))
    # colour: against the float64 formula at the flat normal, with the restatement's own foam (a constant here)
    foam = tex.S(np.zeros((1, 2), f32))[0, 0, 3]
    for mat in (oh.material(foam_threshold=float(foam) + 0.5), oh.material(foam_threshold=float(foam) - 0.5),
                oh.material(light_direction=(0.3, -0.2, 0.5))):
        col = restate_camera(tex, cam, mat, w, h, oh.CAMERA_COLOR, k, steps, refine)
        assert col.dtype == f32 and col.shape == (w * h, 4)
        np.testing.assert_array_equal(col[:, 3], hits[:, 3])
        nh = int(hit.sum())
        want = shade(rays[hit, 3:6], np.tile([0.0, 1.0, 0.0], (nh, 1)), np.zeros(nh), np.full(nh, foam), mat, True,
                     np.float64)
        # (1e-4: the Cook-Torrance distribution's q = ndh^2 (a2 - 1) + 1 cancels to a2 = 0.0081 at the highlight, so
        # fp32 carries a few eps / a2 there)
        np.testing.assert_allclose(col[hit, :3], want, rtol=1e-4, atol=1e-6)
        sat = np.clip(dy[~hit], 0, 1)[:, None]
        m = mat.astype(np.float64)
        np.testing.assert_allclose(col[~hit, :3], m[26:29] + sat * (m[29:32] - m[26:29]), rtol=1e-6)
    plain = oh.material(sun_strength=0.0, subsurface_intensity=0.0, foam_threshold=float(foam) + 0.5,
                        horizon_color=(0.4, 0.5, 0.6), zenith_color=(0.4, 0.5, 0.6), environment_strength=0.8)
    col = restate_camera(tex, cam, plain, w, h, oh.CAMERA_COLOR, k, steps, refine)
    m = plain.astype(np.float64)
    fres = m[3] + (1 - m[3]) * (1 - np.clip(-dy[hit], 0, 1)) ** m[4] / m[5]
    want = m[0:3] + fres[:, None] * (np.pi * 0.8 * m[26:29] - m[0:3])
    np.testing.assert_allclose(col[hit, :3], want, rtol=2e-5)
    # under water: every pixel is the water colour, status SUBMERGED, range t0
    sub = oh.look_at_camera((0.0, -3.0, 0.0), (5.0, 1.0, 5.0), (0, 1, 0), 0.9, w, h, 0.25, 50.0)
    col = restate_camera(tex, sub, plain, w, h, oh.CAMERA_COLOR, k, steps, refine)
    np.testing.assert_array_equal(col, np.tile(np.r_[plain[0:3], f32(oh.RAY_SUBMERGED)], (w * h, 1)))
    np.testing.assert_array_equal(restate_camera(tex, sub, None, w, h, oh.CAMERA_RANGE, k, steps, refine), f32(0.25))


def test_restatement_rounding_yardstick_is_fp32_sized():
    """shade() in fp32 against itself in float64 from the same fp32 inputs: the yardstick of the GPU test.  Over
    random unit normals near the vertical and descending rays it is fp32-sized: a few eps, times the conditioning
    of the Cook-Torrance distribution at the highlight, where q = ndh^2 (a2 - 1) + 1 cancels to a2 = 0.0081 (1 / a2 =
    123, entering twice through ndh^2 and twice through q^2: about 500 eps at the worst pixel)."""
    rng = np.random.default_rng(3)
    m = 2000
    d = rng.normal(size=(m, 3))
    d[:, 1] = -np.abs(d[:, 1]) - 0.05
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    n = np.c_[rng.normal(0, 0.2, m), np.ones(m), rng.normal(0, 0.2, m)]
    n = (n / np.linalg.norm(n, axis=1)[:, None]).astype(f32)
    eta, foam = rng.normal(0, 1, m).astype(f32), rng.uniform(0, 2, m).astype(f32)
    mat = oh.material(roughness=0.3, foam_threshold=1.0)
    a, b = shade(d, n, eta, foam, mat, True, f32), shade(d, n, eta, foam, mat, True, np.float64)
    assert a.dtype == f32 and b.dtype == np.float64 and np.isfinite(b).all()
    rel = np.abs(a - b).max(axis=0) / np.abs(b).max(axis=0)
    print("fp32 restatement against float64, per channel:", rel)
    assert (rel < 1024 * np.finfo(f32).eps).all() and (rel > 0).all()
