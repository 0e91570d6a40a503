"""CPU tests of the camera views in which the water sees the bodies (ocean_camera_scene, _device, _async;
include/ocean/ocean.h): the symbols, the constants, the ctypes signatures, the validation that precedes every device
call (reached with a null context), and restate_camera_scene, the numpy statement of an image that
tests/test_gpu_camera_scene.py compares the kernel with.  The restatement is built on restate_camera_bodies
(tests/test_camera_bodies_abi.py): the primary test, the body pixels and the pixels that are no water HIT pixel are
its own; meet_rays tries every body for every secondary ray, statement by statement as body_pixels does but with an
origin per ray; shade_scene is the camera's shade() with the three terms, written once over a dtype.  All geometry
and every decision (q, rd, the slab tests, sf, b1, b2, te, nw) is fp32 whatever the dtype of the colours.

scene_boxes is the scene of the GPU tests; its constants were chosen here, over the oracle's textures."""
import ctypes
import os

import numpy as np

import atmosphere_ref as A
import ocean_hip as oh
import oracle as O
from test_camera_abi import PI32, TINY32, shading_inputs
from test_camera_bodies_abi import QUIET, UNIT_BOX, body_colour, body_pixels, restate_camera_bodies, rot
from test_ray_abi import _oracle_textures

f32 = np.float32
SYMBOLS = ("ocean_camera_scene", "ocean_camera_scene_device", "ocean_camera_scene_async")
SKY = oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT


# ---------------------------------------------------------------------------- the restatement
def meet_rays(p, r, s0, s1, box, bodies):
    """ocean.h's meet(p, r, s0, s1) for rays with an origin each: p, r [M][3] fp32 -> (b [M], -1 where no body is met;
    te [M]; nw [M][3]), every body tried for every ray in ascending b.  The statements are body_pixels'."""
    p, r = np.ascontiguousarray(p, f32), np.ascontiguousarray(r, f32)
    s0, s1 = f32(s0), f32(s1)
    lo, hi = np.asarray(box, f32)[:3], np.asarray(box, f32)[3:]
    m = len(p)
    best_b, best_te, best_nw = np.full(m, -1), np.full(m, np.inf, f32), np.zeros((m, 3), f32)
    rows = np.arange(m)
    for b, rec in enumerate(np.asarray(bodies, f32).reshape(-1, np.shape(bodies)[-1]) if len(bodies) else ()):
        c, u, qw, s = rec[0:3], rec[3:6], rec[6], rec[7:10]
        ob = rot(-u, qw, p - c[None, :])
        db = rot(-u, qw, r)
        l, h = s * lo, s * hi
        with np.errstate(**QUIET):
            a, e = (l[None, :] - ob) / db, (h[None, :] - ob) / db
        beside = db == 0
        between = (np.minimum(l, h)[None, :] <= ob) & (ob <= np.maximum(l, h)[None, :])
        n = np.where(beside, f32(-np.inf), np.minimum(a, e))
        f = np.where(beside, f32(np.inf), np.maximum(a, e))
        tn = np.maximum(np.maximum(n[:, 0], n[:, 1]), n[:, 2])
        tf = np.minimum(np.minimum(f[:, 0], f[:, 1]), f[:, 2])
        met = (~beside | between).all(axis=1) & (tn <= tf) & (tf >= s0) & (tn <= s1) & (not s1 < s0)
        te = np.maximum(tn, s0)
        axis = (n == tn[:, None]).argmax(axis=1)  # the first of x, y, z
        nb = np.zeros((m, 3), f32)
        nb[rows, axis] = np.where(db[rows, axis] > 0, f32(-1), f32(1))
        nw = np.where((tn >= s0)[:, None], rot(u, qw, nb), -r)
        win = met & (te < best_te)
        best_b[win], best_te[win], best_nw[win] = b, te[win], nw[win]
        assert te.dtype == f32 and nw.dtype == f32 and ob.dtype == f32
    return best_b, best_te, best_nw


def shade_scene(d, n, eta, foam, material, has_foam, terms, dtype=f32, S=None):
    """ocean.h's colour of a water HIT pixel of ocean_camera_scene in `dtype`: the camera's "Colour of a hit"
    (test_camera_abi.shade, or atmosphere_ref.shade_sky with the sky-view table S) with base, src and the shadowed
    composition.  terms: through, mirrored, shadowed [M] bool; depth [M] fp32; seen, mirror [M][3] (paintc in
    `dtype`); optics."""
    t = dtype
    d, n, eta, foam = (np.asarray(a).astype(t) for a in (d, n, eta, foam))
    m = np.asarray(material, f32).astype(t)
    op = np.asarray(terms["optics"], f32).astype(t)
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
    r = (t(2) * ndv)[:, None] * n - V
    if S is None:
        src = hz[None, :] + sat(r[:, 1])[:, None] * (zn - hz)[None, :]
    else:
        src = A.sky_lookup(S, r, t)
    src = np.where(terms["mirrored"][:, None], np.asarray(terms["mirror"]).astype(t), src)
    env = (src * pi) * ke
    fog = np.exp2(-(op[4] * np.asarray(terms["depth"], f32).astype(t)))
    base = np.where(terms["through"][:, None], C[None, :] + fog[:, None] * (np.asarray(terms["seen"]).astype(t) - C[None, :]),
                    C[None, :])
    refraction = base + (g[:, None] * ss[None, :]) * lc[None, :]
    if L[1] > 0:
        den = np.maximum(one - h[:, 2] * h[:, 2], tiny)
        c2, s2 = np.maximum((h[:, 0] * h[:, 0]) / den, zero), np.maximum((h[:, 1] * h[:, 1]) / den, zero)
        nu, nv = (ex * t(10)) * (one - rho), (ey * t(10)) * (one - rho)
        D = np.sqrt((nu + one) * (nv + one)) * np.power(np.maximum(hdn, zero), nu * c2 + nv * s2)
        Ash = np.maximum((D * FH) / np.maximum(((t(8) * pi) * hdv) * np.maximum(ndv, ndl), tiny), zero)
        ash = lc[None, :] * Ash[:, None]
        a2 = (rho * rho) * (rho * rho)
        q = (sat(hdn) * sat(hdn)) * (a2 - one) + one
        N = np.maximum(a2 / np.maximum(pi * (q * q), tiny), zero)
        k = rho / t(2)
        G = np.maximum((sat(ndv) / np.maximum(sat(ndv) * (one - k) + k, tiny)) *
                       (sat(ndl) / np.maximum(sat(ndl) * (one - k) + k, tiny)), zero)
        cook = ((lc[None, :] * N[:, None]) * G[:, None]) / np.maximum((t(8) * sat(ndv)) * sat(ndl), tiny)[:, None]
    else:
        ash = cook = np.zeros((len(d), 3), t)
    shadowed = terms["shadowed"][:, None]
    reflections = np.where(shadowed, env, env + (cook + ash * sat(ndv)[:, None]) * ks)
    e = refraction + F[:, None] * (reflections - refraction)
    e = np.where(shadowed, e + op[3] * (op[None, 0:3] - e), e)
    if has_foam:
        foamy = foam >= ft
        e = np.where(foamy[:, None], e + fb * (fc[None, :] - e), e)
    assert e.dtype == t
    return e


def restate_camera_scene(tex, camera, material, w, h, mode, k, steps, refine, box, paint, optics, bodies, dtype=f32,
                         sky=None):
    """ocean.h's definition of ocean_camera_scene in numpy, operation by operation: the image [h * w][4] and what it
    was composed from (restate_camera_bodies' info, and water: the water HIT pixels; q, rd; sf, b1t, b2 of every
    pixel).  Geometry and decisions are fp32; `dtype` is that of the colours.  sky = (S, sun_size) in the
    OCEAN_CAMERA_SKY_LUT mode."""
    links = mode == oh.CAMERA_LINKS
    base_mode = oh.CAMERA_COLOR if links else mode
    pt = f32([0, 0, 0, 0]) if paint is None else paint
    out, info = restate_camera_bodies(tex, camera, material, w, h, base_mode, k, steps, refine, box, pt, bodies, dtype,
                                      sky)
    rays, rec, hit, n, eta, foam = shading_inputs(tex, camera, material, w, h, k, steps, refine)
    op = np.asarray(optics, f32)
    m = np.asarray(material, f32)
    M = len(rays)
    body, b1, te1, nw1 = info["body"], info["b"], info["te"], info["nw"]
    water = (rec[:, 3] == oh.RAY_HIT) & ~body
    at = np.flatnonzero(water[hit])  # the water pixels among shading_inputs' hit arrays
    wp = hit[at]
    d, tstar = rays[wp, 3:6], rec[wp, 0]
    q = rays[wp, 0:3] + tstar[:, None] * d
    nn = np.ascontiguousarray(n[at], f32)
    V = -d
    ndv = (nn[:, 0] * V[:, 0] + nn[:, 1] * V[:, 1]) + nn[:, 2] * V[:, 2]
    rd = (f32(2) * ndv)[:, None] * nn - V
    assert q.dtype == f32 and rd.dtype == f32
    L = m[20:23]
    if L[1] > 0:
        shadowed = meet_rays(q, np.tile(L, (len(q), 1)), 0.0, op[5], box, bodies)[0] >= 0
    else:
        shadowed = np.zeros(len(q), bool)
    b2w, _, nw2 = meet_rays(q, rd, 0.0, op[5], box, bodies)
    sf, b1t, b2 = np.ones(M, f32), np.full(M, -1), np.full(M, -1)
    sf[wp], b1t[wp], b2[wp] = np.where(shadowed, f32(0), f32(1)), b1[wp], b2w
    info.update(water=water, q=q, rd=rd, sf=sf, b1t=b1t, b2=b2, wp=wp)
    if links:
        out = np.empty((M, 4), f32)
        out[:, 0], out[:, 1], out[:, 2] = 1, np.where(body, b1, -1), -1
        out[:, 3] = np.where(body, oh.RAY_BODY, rec[:, 3])
        out[wp, 0], out[wp, 1], out[wp, 2] = sf[wp], b1t[wp], b2[wp]
        return out, info
    S = None if mode == oh.CAMERA_COLOR else sky[0]
    terms = dict(optics=op, through=b1[wp] >= 0, mirrored=b2w >= 0, shadowed=shadowed,
                 depth=np.where(b1[wp] >= 0, te1[wp] - tstar, f32(0)).astype(f32),
                 seen=body_colour(nw1[wp], material, paint, dtype, S), mirror=body_colour(nw2, material, paint, dtype, S))
    out[wp, :3] = shade_scene(d, nn, eta[at], foam[at], material, tex.deriv is not None, terms, dtype, S)
    return out, info


# ---------------------------------------------------------------------------- the scene of the GPU tests
BOX = f32([-0.5, -0.25, -0.5, 0.5, 0.75, 0.5])  # tests/test_gpu_camera_bodies.py's
PAINT = f32([0.85, 0.35, 0.15, 0.6])
SUN = (-0.55, 0.33, 0.35)  # low (19 degrees up) and from the left: the shadows run across the view
OPTICS = oh.optics(shadow_color=(0.02, 0.03, 0.08), shadow_intensity=0.6, fog_density=0.15, reach=120.0)


def oracle_bounds(tex):
    """ocean_surface_bounds over the textures: [C][8] = (min x, y, z, w, max x, y, z, w) of each DISP slice."""
    C = len(tex.lengths)
    flat = tex.disp.reshape(C, -1, 4)
    return np.concatenate([flat.min(axis=1), flat.max(axis=1)], axis=1).astype(f32)


def scene_boxes(cam, bounds, w, h, stride=10):
    """The bodies of the scene: test_gpu_camera_bodies.scatter_boxes(cam, 300), the sunk box and the near box of its
    test_time_only_switches_change_no_bit (302 records), and behind them four tall boxes standing in the water 25 to
    90 m ahead, which throw long shadows under SUN, stand in their own reflections and reach 5 m under the surface."""
    from test_gpu_camera_bodies import scatter_boxes
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (w - 1) / 2 + c[9:12] * (h - 1) / 2
    low = float(bounds[:, 1].astype(np.float64).sum())
    sunk = np.r_[c[0:3] + 35.0 * ahead, 0, 0, 0, 1, 30, 2, 30]
    sunk[1] = low - 4.0
    air = np.r_[c[0:3] + 8.0 * ahead + [0.0, -0.4, 0.0], 0, 0.6, 0, 0.8, 1.8, 1.1, 0.9]
    flat = np.float64([ahead[0], 0.0, ahead[2]])
    flat /= np.linalg.norm(flat)
    side = np.float64([flat[2], 0.0, -flat[0]])
    tall = []
    for dist, off, turn, size in ((25.0, -4.0, 0.2, (2.5, 20.0, 2.5)), (45.0, 9.0, -0.5, (4.0, 20.0, 4.0)),
                                  (65.0, -14.0, 0.9, (5.0, 24.0, 5.0)), (90.0, 6.0, 0.0, (7.0, 28.0, 7.0))):
        at = c[0:3] + dist * flat + off * side
        tall.append(np.r_[at[0], 0.0, at[2], 0.0, np.sin(turn / 2), 0.0, np.cos(turn / 2), size])
    rec = np.random.default_rng(11).uniform(-1e3, 1e3, (306, stride))  # junk behind the tenth float
    rec[:300, :10] = scatter_boxes(cam, 300)
    rec[300:, :10] = np.float64([sunk, air] + tall)
    return rec.astype(f32)


def link_shares(info):
    """What the restatement's image holds: the water HIT pixels that are shadowed, that show a body through the water,
    that reflect one, and that have no link at all; and the largest linked body index."""
    wp = info["wp"]
    sf, b1t, b2 = info["sf"][wp], info["b1t"][wp], info["b2"][wp]
    return dict(water=len(wp), shadowed=int((sf == 0).sum()), through=int((b1t >= 0).sum()),
                mirrored=int((b2 >= 0).sum()), free=int(((sf == 1) & (b1t < 0) & (b2 < 0)).sum()),
                top=int(max(b1t.max(initial=-1), b2.max(initial=-1))))


def check_link_shares(info):
    s = link_shares(info)
    print(s)
    assert s["shadowed"] >= 20 and s["through"] >= 20 and s["mirrored"] >= 20 and s["free"] >= 20 and s["top"] >= 256, s


# ---------------------------------------------------------------------------- the ABI
def test_camera_scene_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.CAMERA_LINKS, oh.SCENE_OPTICS_FLOATS) == (3, 6)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sig = [P, i, i, i, i, i, P, P, i, i, P, P, P, P, i, i, P, sz]
    for name, args in ((SYMBOLS[0], sig), (SYMBOLS[1], sig), (SYMBOLS[2], sig + [ctypes.POINTER(P)])):
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("camera_scene", "camera_scene_async", "camera_scene_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.camera_scene)
    op = oh.optics(shadow_color=(0.1, 0.2, 0.3), shadow_intensity=0.7, fog_density=0.25, reach=40.0)
    assert op.dtype == f32
    np.testing.assert_array_equal(op, f32([0.1, 0.2, 0.3, 0.7, 0.25, 40.0]))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ocean", "ocean.h")).read()
    assert "#define OCEAN_CAMERA_LINKS 3 " in header and "#define OCEAN_SCENE_OPTICS_FLOATS 6\n" in header
    assert "ocean_camera_scene_async" in header.split("#define OCEAN_ABI_VERSION 4")[0]  # the version history names it


def _call(L, name, kw):
    """One entry with the arguments `kw` over a valid base; (code, message, req after the call or "no req")."""
    cam = np.ascontiguousarray(kw.get("camera", oh.look_at_camera((0, 10, 0), (0, 0, 30), (0, 1, 0), 0.8, 4, 3, 0, 90)))
    mat = kw.get("material", oh.material())
    box, paint = kw.get("box", UNIT_BOX), kw.get("paint", f32([0.8, 0.7, 0.6, 1.0]))
    optics = kw.get("optics", oh.optics())
    stride, count = kw.get("stride", 10), kw.get("count", 2)
    bodies = np.tile(f32([0, 0, 20, 0, 0, 0, 1, 1, 1, 1] + [0] * 54), 2)
    w, h, mode = kw.get("width", 4), kw.get("height", 3), kw.get("mode", oh.CAMERA_COLOR)
    nbytes = kw.get("bytes", w * h * 16)
    out = np.zeros(4 * 3 * 8, f32)
    vp = ctypes.c_void_p
    args = [None, kw.get("tile", 0), mode, kw.get("iterations", 2), kw.get("steps", 16), kw.get("refine", 4),
            None if kw.get("null_camera") else vp(cam.ctypes.data), None if mat is None else vp(mat.ctypes.data), w, h,
            None if box is None else vp(box.ctypes.data), None if paint is None else vp(paint.ctypes.data),
            None if optics is None else vp(optics.ctypes.data),
            None if kw.get("null_bodies") else vp(bodies.ctypes.data + kw.get("misalign_bodies", 0)), stride, count,
            None if kw.get("null_out") else vp(out.ctypes.data + kw.get("misalign", 0)), nbytes]
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)  # (leaves another message behind)
    rc = getattr(L, name)(*args, *((ctypes.byref(req),) if name.endswith("_async") else ()))
    assert not out.any()
    return rc, L.ocean_last_error().decode(), req.value if name.endswith("_async") else "no req"


def _optics(k, value):
    op = oh.optics()
    op[k] = value
    return op


# its own refusals ...
BAD = [(dict(optics=None), "null optics"), (dict(optics=None, mode=oh.CAMERA_LINKS), "null optics"),
       (dict(optics=_optics(0, np.nan)), "optics[0]"), (dict(optics=_optics(3, np.inf)), "optics[3]"),
       (dict(optics=_optics(4, -np.inf), mode=oh.CAMERA_LINKS), "optics[4]"), (dict(optics=_optics(5, np.nan)), "optics[5]"),
       (dict(optics=_optics(5, -1.0)), "reach"), (dict(optics=_optics(5, -1e-30), mode=oh.CAMERA_LINKS), "reach"),
       (dict(mode=oh.CAMERA_HITS, bytes=4 * 3 * 32), "mode"), (dict(mode=oh.CAMERA_RANGE, bytes=4 * 3 * 4), "mode"),
       (dict(mode=oh.CAMERA_HITS), "mode"), (dict(mode=oh.CAMERA_RANGE), "mode"),
       (dict(mode=oh.CAMERA_LINKS | oh.CAMERA_SKY_LUT), "mode"), (dict(mode=4), "mode"), (dict(mode=-1), "mode"),
       (dict(paint=None), "paint"), (dict(paint=None, mode=SKY), "paint"),
       (dict(material=None), "material"), (dict(material=None, mode=SKY), "material"),
       (dict(material=None, mode=oh.CAMERA_LINKS), "material"),
       (dict(bytes=4 * 3 * 16 - 4), "byte count"), (dict(bytes=4 * 3 * 32, mode=oh.CAMERA_LINKS), "byte count"),
       (dict(bytes=0, mode=SKY), "byte count"),
       # ... and a sample of what ocean_camera_bodies* refuses (the tests are its own)
       (dict(null_camera=True), "null camera"), (dict(null_out=True), "null camera or output"),
       (dict(steps=0), "steps"), (dict(refine=33), "refine"), (dict(iterations=17), "iterations"),
       (dict(width=0), "width"), (dict(box=None), "null box"),
       (dict(box=np.r_[UNIT_BOX[:5], np.nan].astype(f32)), "box[5]"),
       (dict(paint=f32([np.nan, 0.5, 0.5, 1.0]), mode=oh.CAMERA_LINKS), "paint[0]"),  # passed: checked
       (dict(stride=9), "stride"), (dict(stride=65), "stride"), (dict(count=-1), "count"),
       (dict(count=oh.BODY_MAX_BODIES + 1), "count"), (dict(null_bodies=True), "null bodies")]


def test_camera_scene_validation_precedes_every_device_call():
    """No GPU here: each case returns OCEAN_E_INVALID_ARG with the argument's name, in all three forms, and *req is
    NULL afterwards.  Valid arguments reach the context test, which refuses the null context."""
    L = oh.load_library()
    for name in SYMBOLS:
        for kw, word in BAD:
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and word in msg, (name, kw, msg)
            assert req in (None, "no req"), (name, kw)
        for kw in (dict(), dict(mode=SKY), dict(mode=oh.CAMERA_LINKS), dict(mode=oh.CAMERA_LINKS, paint=None),
                   dict(optics=_optics(5, 0.0)), dict(count=0, null_bodies=True), dict(stride=64)):
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and "context" in msg, (name, kw, msg)
            assert req in (None, "no req")
    for kw in (dict(misalign=4), dict(misalign_bodies=2)):
        rc, msg, _ = _call(L, "ocean_camera_scene_device", kw)
        assert rc == oh.E_INVALID_ARG and "aligned" in msg and "ocean_camera_scene" in msg, (kw, msg)
        rc, msg, _ = _call(L, "ocean_camera_scene", kw)  # a host buffer needs no alignment
        assert "context" in msg
    # ocean_camera* and ocean_camera_bodies* still refuse the new mode
    cam, mat, out = oh.look_at_camera((0, 10, 0), (0, 0, 30), (0, 1, 0), 0.8, 4, 3, 0, 90), oh.material(), np.zeros(48, f32)
    assert L.ocean_camera(None, 0, oh.CAMERA_LINKS, 2, 16, 4, cam.ctypes.data, mat.ctypes.data, 4, 3, out.ctypes.data,
                          192) == oh.E_INVALID_ARG and b"mode" in L.ocean_last_error()
    assert L.ocean_camera_bodies(None, 0, oh.CAMERA_LINKS, 2, 16, 4, cam.ctypes.data, mat.ctypes.data, 4, 3,
                                 UNIT_BOX.ctypes.data, PAINT.ctypes.data, None, 10, 0, out.ctypes.data,
                                 192) == oh.E_INVALID_ARG and b"mode" in L.ocean_last_error()


# ---------------------------------------------------------------------------- known answers
def test_meet_rays_is_body_pixels_with_an_origin_per_ray():
    """From one origin meet_rays equals body_pixels bit for bit; a shadow ray from under a box meets it, one from
    beside it or with a reach that ends below it does not; a ray that starts inside a box has te = 0 and nw = -r."""
    rng = np.random.default_rng(5)
    d = rng.normal(size=(200, 3))
    d = (d / np.linalg.norm(d, axis=1)[:, None]).astype(f32)
    q = rng.normal(size=(40, 4))
    bodies = np.c_[rng.uniform(-20, 20, (40, 3)), q / np.linalg.norm(q, axis=1)[:, None], rng.uniform(1, 9, (40, 3))].astype(f32)
    rays = np.empty((200, 8), f32)
    rays[:, 0:3], rays[:, 3:6], rays[:, 6], rays[:, 7] = (1, 2, 3), d, 0.5, 30.0
    want = body_pixels(rays, BOX, bodies)
    got = meet_rays(rays[:, 0:3], d, 0.5, 30.0, BOX, bodies)
    assert (want[0] >= 0).sum() >= 50 and (want[0] < 0).sum() >= 20
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    box = np.r_[0, 10, 0, 0, 0, 0, 1, 4, 2, 4].astype(f32)  # y from 9 to 11 over the square |x|, |z| <= 2
    p = f32([[0, 0, 0], [1.9, 0, 0], [2.1, 0, 0], [0, 0, 0], [0, 10, 0]])
    up = np.tile(f32([0, 1, 0]), (5, 1))
    b, te, nw = meet_rays(p, up, 0.0, 50.0, UNIT_BOX, [box])
    np.testing.assert_array_equal(b, [0, 0, -1, 0, 0])
    np.testing.assert_array_equal(te[[0, 1, 4]], f32([9, 9, 0]))
    np.testing.assert_array_equal(nw[[0, 4]], [[0, -1, 0], [0, -1, 0]])
    assert meet_rays(p[:1], up[:1], 0.0, 8.5, UNIT_BOX, [box])[0][0] == -1  # the reach ends below the box
    assert meet_rays(p[:1], up[:1], 0.0, 9.0, UNIT_BOX, [box])[0][0] == 0   # the bound is met
    assert meet_rays(p[:1], up[:1], 0.0, 0.0, UNIT_BOX, [box])[0][0] == -1 and meet_rays(p[4:], up[4:], 0, 0, UNIT_BOX, [box])[0][0] == 0
    assert meet_rays(p, up, 0.0, 50.0, UNIT_BOX, [])[0].max() == -1


def _oracle_scene(n=64, ncasc=1):
    cas = O.SCENE_CASCADES[:ncasc]
    tex = _oracle_textures(n, cas, O.generate_noise(n, 20251121))
    from test_gpu_camera import H, K, REFINE, STEPS, W, pose_above
    bounds = oracle_bounds(tex)
    cam = pose_above(bounds)
    return tex, cam, bounds, (W, H, K, STEPS, REFINE)


def test_scene_of_the_gpu_tests_has_every_link_on_the_oracle_textures():
    """The constants of scene_boxes, SUN and OPTICS, over the oracle's textures of the first GPU context: every kind of
    link is there, a body of the second chunk among them; the LINKS image says the same as the info."""
    tex, cam, bounds, (W, H, K, STEPS, REFINE) = _oracle_scene()
    bodies = scene_boxes(cam, bounds, W, H)
    mat = oh.material(roughness=0.3, light_direction=SUN)
    links, info = restate_camera_scene(tex, cam, mat, W, H, oh.CAMERA_LINKS, K, STEPS, REFINE, BOX, None, OPTICS, bodies)
    check_link_shares(info)
    assert links.dtype == f32 and links.shape == (W * H, 4)
    water = info["water"]
    np.testing.assert_array_equal(links[water, 3], oh.RAY_HIT)
    np.testing.assert_array_equal(links[~water, 0], 1)
    np.testing.assert_array_equal(links[~water, 2], -1)
    np.testing.assert_array_equal(links[info["body"], 1], info["b"][info["body"]])
    assert set(np.unique(links[:, 0])) == {0.0, 1.0}


def test_no_bodies_is_restate_camera_bodies_and_a_blind_scene_differs_inside_boxes_only():
    """count == 0: restate_camera_bodies' image bit for bit.  SI = 0, WF large and reach = 0: no fog shows a body, the
    shadow changes no colour, and a secondary ray of no length meets a box only from inside it: the pixels that differ
    from restate_camera_bodies' all have their q inside a box (by the fp32 slab test of a zero-length ray)."""
    tex, cam, bounds, (W, H, K, STEPS, REFINE) = _oracle_scene()
    mat = oh.material(roughness=0.3, light_direction=SUN)
    for bodies in ([], np.zeros((0, 10), f32)):
        got, _ = restate_camera_scene(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, OPTICS, bodies)
        want, _ = restate_camera_bodies(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, bodies)
        np.testing.assert_array_equal(got, want)
    bodies = scene_boxes(cam, bounds, W, H)
    blind = oh.optics(shadow_color=(0.3, 0.2, 0.1), shadow_intensity=0.0, fog_density=1.0e6, reach=0.0)
    got, info = restate_camera_scene(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, blind, bodies)
    want, _ = restate_camera_bodies(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, bodies)
    differ = (got != want).any(axis=1)
    wp = info["wp"]
    inside = np.zeros(W * H, bool)
    sun = np.tile(mat[20:23], (len(wp), 1))
    inside[wp] = (meet_rays(info["q"], info["rd"], 0.0, 0.0, BOX, bodies)[0] >= 0) | \
        (meet_rays(info["q"], sun, 0.0, 0.0, BOX, bodies)[0] >= 0)
    print(f"{differ.sum()} pixels differ, {inside.sum()} water pixels lie inside a box")
    assert not (differ & ~inside).any()  # (a box that holds q is in front of it: such pixels are rare or absent)
    np.testing.assert_array_equal(got[:, 3], want[:, 3])
    # with the scene's own optics many pixels differ, the linked ones among them, and no others
    got, info = restate_camera_scene(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, OPTICS, bodies)
    linked = (info["sf"] == 0) | (info["b1t"] >= 0) | (info["b2"] >= 0)
    differ = (got != want).any(axis=1)
    assert not (differ & ~linked).any() and differ.sum() >= 40
    got64, _ = restate_camera_scene(tex, cam, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE, BOX, PAINT, OPTICS, bodies,
                                    np.float64)
    assert got.dtype == f32 and got64.dtype == np.float64
    np.testing.assert_allclose(got[:, :3], got64[:, :3], rtol=2e-3, atol=1e-5)
