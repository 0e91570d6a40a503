"""CPU tests of the camera views that see the bodies (ocean_camera_bodies, _device, _async; include/ocean/ocean.h):
the symbols, the constants, the ctypes signatures, the validation that precedes every device call (reached with a
null context, as tests/test_camera_abi.py does), and restate_camera_bodies, the numpy fp32 statement of an image that
tests/test_gpu_camera_bodies.py compares the kernel with.  The restatement is built on restate_camera's parts: the
water's records and colours are theirs, and body_pixels brute-forces every body per pixel, statement by statement;
body_colour is written once over a dtype, so the same statements give the fp32 restatement and its float64 twin.
Here the slab test meets boxes whose answers are known in closed form, and a flat sea hides and shows a box."""
import ctypes
import os

import numpy as np

import atmosphere_ref as A
import ocean_hip as oh
from test_camera_abi import _flat, camera_rays, colours, shading_inputs

f32 = np.float32
SYMBOLS = ("ocean_camera_bodies", "ocean_camera_bodies_device", "ocean_camera_bodies_async")
PIXEL_FLOATS = {oh.CAMERA_HITS: 8, oh.CAMERA_RANGE: 1, oh.CAMERA_COLOR: 4, oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT: 4}
UNIT_BOX = f32([-0.5, -0.5, -0.5, 0.5, 0.5, 0.5])
QUIET = dict(divide="ignore", invalid="ignore", over="ignore")


# ---------------------------------------------------------------------------- the restatement
def _cross(p, q):
    return np.stack([p[..., 1] * q[..., 2] - p[..., 2] * q[..., 1], p[..., 2] * q[..., 0] - p[..., 0] * q[..., 2],
                     p[..., 0] * q[..., 1] - p[..., 1] * q[..., 0]], axis=-1)


def rot(u, w, a):
    """ocean.h's rot(u, w, a): t = 2 (u x a), (a + w t) + (u x t); u [3], w scalar, a [..][3], all fp32."""
    t = f32(2) * _cross(u, a)
    out = (a + w * t) + _cross(u, t)
    assert out.dtype == f32
    return out


def body_pixels(rays, box, bodies):
    """ocean.h's body of every pixel: rays [M][8] (one o, t0, t1 for all) and records [count][>= 10] ->
    (b [M], -1 where no body is met; te [M]; nw [M][3]), all fp32, every body tried for every pixel in ascending b."""
    rays = np.ascontiguousarray(rays, f32)
    o, d, t0, t1 = rays[0, 0:3], rays[:, 3:6], rays[0, 6], rays[0, 7]
    lo, hi = np.asarray(box, f32)[:3], np.asarray(box, f32)[3:]
    m = len(rays)
    best_b, best_te, best_nw = np.full(m, -1), np.full(m, np.inf, f32), np.zeros((m, 3), f32)
    rows = np.arange(m)
    for b, rec in enumerate(np.asarray(bodies, f32).reshape(-1, np.shape(bodies)[-1]) if len(bodies) else ()):
        c, u, qw, s = rec[0:3], rec[3:6], rec[6], rec[7:10]
        ob = rot(-u, qw, o - c)
        db = rot(-u, qw, d)
        l, h = s * lo, s * hi
        with np.errstate(**QUIET):
            a, e = (l - ob)[None, :] / db, (h - ob)[None, :] / db
        beside = db == 0
        between = (np.minimum(l, h) <= ob) & (ob <= np.maximum(l, h))
        n = np.where(beside, f32(-np.inf), np.minimum(a, e))
        f = np.where(beside, f32(np.inf), np.maximum(a, e))
        tn = np.maximum(np.maximum(n[:, 0], n[:, 1]), n[:, 2])
        tf = np.minimum(np.minimum(f[:, 0], f[:, 1]), f[:, 2])
        met = (~beside | between[None, :]).all(axis=1) & (tn <= tf) & (tf >= t0) & (tn <= t1) & (not t1 < t0)
        te = np.maximum(tn, t0)
        axis = (n == tn[:, None]).argmax(axis=1)  # the first of x, y, z
        nb = np.zeros((m, 3), f32)
        nb[rows, axis] = np.where(db[rows, axis] > 0, f32(-1), f32(1))
        nw = np.where((tn >= t0)[:, None], rot(u, qw, nb), -d)
        win = met & (te < best_te)
        best_b[win], best_te[win], best_nw[win] = b, te[win], nw[win]
        assert te.dtype == f32 and nw.dtype == f32
    return best_b, best_te, best_nw


def body_colour(nw, material, paint, dtype=f32, S=None):
    """A body pixel's rgb in `dtype` from its fp32 normal: A_c (ka amb_c + LC_c max(dot(nw, L), 0)); S: the sky-view
    table of OCEAN_CAMERA_SKY_LUT, else the two-colour sky."""
    t = dtype
    m, p, n = np.asarray(material, f32).astype(t), np.asarray(paint, f32).astype(t), np.asarray(nw).astype(t)
    L, lc, hz, zn = m[20:23], m[23:26], m[26:29], m[29:32]
    if S is None:
        sat = np.minimum(np.maximum(n[:, 1], t(0)), t(1))
        amb = hz[None, :] + sat[:, None] * (zn - hz)[None, :]
    else:
        amb = A.sky_lookup(S, n, t)
    lit = np.maximum((n[:, 0] * L[0] + n[:, 1] * L[1]) + n[:, 2] * L[2], t(0))
    out = p[None, :3] * (p[3] * amb + lc[None, :] * lit[:, None])
    assert out.dtype == t
    return out


def compose(rec, b, te):
    """Which pixels are body pixels: a body is met and the water's record is a MISS, or a HIT further than te."""
    return (b >= 0) & ((rec[:, 3] == oh.RAY_MISS) | ((rec[:, 3] == oh.RAY_HIT) & (te < rec[:, 0])))


def restate_camera_bodies(tex, camera, material, w, h, mode, k, steps, refine, box, paint, bodies, dtype=f32, sky=None):
    """ocean.h's definition of ocean_camera_bodies in numpy, operation by operation: the image ([h * w][8], [h * w] or
    [h * w][4]) and what it was composed from (rec: the water's records, b, te: every pixel's body, body: the body
    pixels).  Geometry is fp32; `dtype` is that of the colours.  sky = (S, sun_size) in the OCEAN_CAMERA_SKY_LUT mode."""
    colour = mode in (oh.CAMERA_COLOR, oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT)
    args = shading_inputs(tex, camera, material if colour else oh.material(), w, h, k, steps, refine)
    rays, rec = args[0], args[1]
    b, te, nw = body_pixels(rays, box, bodies)
    body = compose(rec, b, te)
    info = dict(rec=rec, b=b, te=te, nw=nw, body=body)
    if mode == oh.CAMERA_HITS:
        out = rec.copy()
        out[body, 0], out[body, 1:3], out[body, 3] = te[body], 0, oh.RAY_BODY
        out[body, 4:7], out[body, 7] = nw[body], b[body]
    elif mode == oh.CAMERA_RANGE:
        out = np.where(rec[:, 3] == oh.RAY_MISS, f32(np.inf), rec[:, 0]).astype(f32)
        out[body] = te[body]
    else:
        has_foam = tex.deriv is not None
        if mode == oh.CAMERA_COLOR:
            out = colours(*args, material, has_foam, dtype)
        else:
            out = A.sky_colours(*args, material, has_foam, sky[0], sky[1], dtype)[0]
        out[body, :3] = body_colour(nw[body], material, paint, dtype, None if mode == oh.CAMERA_COLOR else sky[0])
        out[body, 3] = oh.RAY_BODY
    return out, info


# ---------------------------------------------------------------------------- the ABI
def test_camera_bodies_symbols_constants_and_signatures():
    L = oh.load_library()
    for s in SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.RAY_BODY, oh.BODY_PAINT_FLOATS, oh.BODY_STRIDE_MIN, oh.BODY_STRIDE_MAX) == (3, 4, 10, 64)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    P, i, sz = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    sig = [P, i, i, i, i, i, P, P, i, i, P, P, P, i, i, P, sz]
    for name, args in ((SYMBOLS[0], sig), (SYMBOLS[1], sig), (SYMBOLS[2], sig + [ctypes.POINTER(P)])):
        fn = getattr(L, name)
        assert list(fn.argtypes) == args and fn.restype is i, name
    for name in ("camera_bodies", "camera_bodies_async", "camera_bodies_device"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.camera_bodies)
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ocean", "ocean.h")).read()
    assert "#define OCEAN_RAY_BODY 3\n" in header and "#define OCEAN_BODY_PAINT_FLOATS 4\n" in header


def _call(L, name, kw):
    """One entry with the arguments `kw` over a valid base; (code, message, req after the call or "no req")."""
    cam = np.ascontiguousarray(kw.get("camera", oh.look_at_camera((0, 10, 0), (0, 0, 30), (0, 1, 0), 0.8, 4, 3, 0, 90)))
    mat = kw.get("material", oh.material())
    box, paint = kw.get("box", UNIT_BOX), kw.get("paint", f32([0.8, 0.7, 0.6, 1.0]))
    stride, count = kw.get("stride", 10), kw.get("count", 2)
    bodies = np.tile(f32([0, 0, 20, 0, 0, 0, 1, 1, 1, 1] + [0] * 54), 2)
    w, h, mode = kw.get("width", 4), kw.get("height", 3), kw.get("mode", oh.CAMERA_COLOR)
    nbytes = kw.get("bytes", w * h * 4 * PIXEL_FLOATS.get(mode, 0))
    out = np.zeros(4 * 3 * 8, f32)
    vp = ctypes.c_void_p
    args = [None, kw.get("tile", 0), mode, kw.get("iterations", 2), kw.get("steps", 16), kw.get("refine", 4),
            None if kw.get("null_camera") else vp(cam.ctypes.data), None if mat is None else vp(mat.ctypes.data), w, h,
            None if box is None else vp(box.ctypes.data), None if paint is None else vp(paint.ctypes.data),
            None if kw.get("null_bodies") else vp(bodies.ctypes.data + kw.get("misalign_bodies", 0)), stride, count,
            None if kw.get("null_out") else vp(out.ctypes.data + kw.get("misalign", 0)), nbytes]
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)  # (leaves another message behind)
    rc = getattr(L, name)(*args, *((ctypes.byref(req),) if name.endswith("_async") else ()))
    assert not out.any()
    return rc, L.ocean_last_error().decode(), req.value if name.endswith("_async") else "no req"


# everything ocean_camera* refuses (a sample of tests/test_camera_abi.py's list: the tests are the camera's own) ...
BAD = [(dict(null_camera=True), "null camera"), (dict(null_out=True), "null camera or output"),
       (dict(material=None), "material"), (dict(mode=3), "mode"), (dict(mode=oh.CAMERA_HITS | oh.CAMERA_SKY_LUT), "mode"),
       (dict(iterations=17), "iterations"), (dict(steps=0), "steps"), (dict(refine=33), "refine"),
       (dict(camera=np.r_[np.zeros(13), np.inf].astype(f32)), "camera[13]"),
       (dict(material=np.r_[np.zeros(31), -np.inf].astype(f32)), "material[31]"),
       (dict(width=0), "width"), (dict(height=-1), "height"),
       (dict(width=1 << 16, height=1 << 16, steps=1), "OCEAN_CAMERA_MAX_PIXELS"),
       (dict(width=1 << 11, height=1 << 11, steps=65), "OCEAN_CAMERA_MAX_SAMPLES"),
       (dict(bytes=4 * 3 * 16 - 4), "byte count"), (dict(mode=oh.CAMERA_RANGE, bytes=4 * 3 * 16), "byte count"),
       # ... and its own
       (dict(box=None), "null box"), (dict(paint=None), "paint"),
       (dict(paint=None, mode=oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT), "paint"),
       (dict(box=np.r_[UNIT_BOX[:5], np.nan].astype(f32)), "box[5]"),
       (dict(box=np.r_[-np.inf, UNIT_BOX[1:]].astype(f32), mode=oh.CAMERA_RANGE), "box[0]"),
       (dict(paint=f32([0.5, 0.5, 0.5, np.inf])), "paint[3]"),
       (dict(paint=f32([np.nan, 0.5, 0.5, 1.0]), mode=oh.CAMERA_HITS, material=None), "paint[0]"),  # passed: checked
       (dict(stride=9), "stride"), (dict(stride=65), "stride"), (dict(stride=0), "stride"), (dict(stride=-10), "stride"),
       (dict(count=-1), "count"), (dict(count=oh.BODY_MAX_BODIES + 1), "count"), (dict(null_bodies=True), "null bodies")]


def test_camera_bodies_validation_precedes_every_device_call():
    """No GPU here: each case returns OCEAN_E_INVALID_ARG with the argument's name, in all three forms, and *req is
    NULL afterwards.  Valid arguments reach the context test, which refuses the null context."""
    L = oh.load_library()
    for name in SYMBOLS:
        for kw, word in BAD:
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and word in msg, (name, kw, msg)
            assert req in (None, "no req"), (name, kw)
        for kw in (dict(), dict(mode=oh.CAMERA_HITS, material=None, paint=None),
                   dict(mode=oh.CAMERA_RANGE, material=None, paint=None), dict(count=0, null_bodies=True),
                   dict(stride=64), dict(stride=32, count=oh.BODY_MAX_BODIES, null_bodies=False),
                   dict(mode=oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT)):  # the limits themselves, and an empty list
            rc, msg, req = _call(L, name, kw)
            assert rc == oh.E_INVALID_ARG and "context" in msg, (name, kw, msg)
            assert req in (None, "no req")
    for kw in (dict(misalign=4), dict(misalign_bodies=2)):
        rc, msg, _ = _call(L, "ocean_camera_bodies_device", kw)
        assert rc == oh.E_INVALID_ARG and "aligned" in msg and "bodies" in msg, (kw, msg)
        rc, msg, _ = _call(L, "ocean_camera_bodies", kw)  # a host buffer needs no alignment
        assert "context" in msg
    rc, msg, _ = _call(L, "ocean_camera_bodies_device", dict(misalign_bodies=2, count=0))  # not read, not checked
    assert "context" in msg
    cam, out = np.zeros(14, f32), np.zeros(16, f32)
    assert L.ocean_camera_bodies_async(None, 0, oh.CAMERA_RANGE, 0, 1, 0, cam.ctypes.data, None, 2, 2,
                                       UNIT_BOX.ctypes.data, None, None, 10, 0, out.ctypes.data, 16, None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


# ---------------------------------------------------------------------------- known answers of the slab test
def _rays(o, dirs, t0=0.0, t1=100.0):
    d = np.atleast_2d(np.asarray(dirs, np.float64))
    d = d / np.linalg.norm(d, axis=1)[:, None]
    r = np.empty((len(d), 8), f32)
    r[:, 0:3], r[:, 3:6], r[:, 6], r[:, 7] = o, d, t0, t1
    return r


def _body(c, q=(0, 0, 0, 1), s=(1, 1, 1)):
    return np.r_[c, q, s].astype(f32)


def test_axis_aligned_box_straight_ahead():
    """A unit box five ahead: the front face at 4.5, its normal towards the eye; scaled (2, 1, 4) the face is at 3.
    A ray a little off the axis meets the same face at 4.5 / d.z; one that passes beside the box meets nothing, nor
    does a search interval that ends in front of it or starts behind it."""
    rays = _rays((0, 0, 0), [(0, 0, 1), (0.05, -0.02, 1), (0.2, 0, 1)])
    b, te, nw = body_pixels(rays, UNIT_BOX, [_body((0, 0, 5))])
    np.testing.assert_array_equal(b, [0, 0, -1])
    assert te[0] == f32(4.5) and abs(float(te[1]) - 4.5 / float(rays[1, 5])) < 1e-6
    np.testing.assert_array_equal(nw[:2], [[0, 0, -1], [0, 0, -1]])
    b, te, nw = body_pixels(rays[:1], UNIT_BOX, [_body((0, 0, 5), s=(2, 1, 4))])
    assert b[0] == 0 and te[0] == f32(3.0)
    off_centre = f32([0, 0, 1, 1, 1, 2])  # a box that does not hold the body's origin
    b, te, nw = body_pixels(_rays((0.5, 0.5, 0), (0, 0, 1)), off_centre, [_body((0, 0, 5), s=(1, 1, 3))])
    assert b[0] == 0 and te[0] == f32(8.0)
    for t0, t1 in ((0.0, 4.0), (5.75, 100.0), (50.0, 10.0)):  # ends in front; starts behind; t1 < t0
        assert body_pixels(_rays((0, 0, 0), (0, 0, 1), t0, t1), UNIT_BOX, [_body((0, 0, 5))])[0][0] == -1
    b, te, _ = body_pixels(_rays((0, 0, 0), (0, 0, 1), 4.5, 5.5), UNIT_BOX, [_body((0, 0, 5))])  # the bounds are met
    assert b[0] == 0 and te[0] == f32(4.5)


def test_ray_parallel_to_a_face_inside_and_outside_the_slab():
    """d = (0, 0, 1) has db.x = db.y = 0 exactly: the body is met iff o lies between the x and y faces (the faces
    included), and the z slabs alone give te."""
    for ox, want in ((0.2, 0), (0.5, 0), (-0.5, 0), (0.7, -1), (-0.500001, -1)):
        b, te, nw = body_pixels(_rays((ox, 0.1, 0), (0, 0, 1)), UNIT_BOX, [_body((0, 0, 5))])
        assert b[0] == want, ox
        if want == 0:
            assert te[0] == f32(4.5) and tuple(nw[0]) == (0, 0, -1)
    b, te, nw = body_pixels(_rays((0.2, 3.0, 0), (0, -1, 0)), UNIT_BOX, [_body((0, 0, 0), s=(1, 2, 1))])  # from above
    assert b[0] == 0 and te[0] == f32(2.0) and tuple(nw[0]) == (0, 1, 0)


def test_eye_inside_the_box():
    """tn < t0: te = t0 and the normal is -d, whatever the face behind the eye."""
    rays = _rays((0.1, -0.2, 5.2), [(0, 0, 1), (1, 2, -0.5)], t0=0.25)
    b, te, nw = body_pixels(rays, UNIT_BOX, [_body((0, 0, 5))])
    np.testing.assert_array_equal(b, [0, 0])
    np.testing.assert_array_equal(te, f32([0.25, 0.25]))
    np.testing.assert_array_equal(nw, -rays[:, 3:6])


def test_quaternion_turns_the_box():
    """A plank (4, 1, 1) seen along z from ten away: across the view its front is the z face at 9.5; turned 90 degrees
    about y it points at the eye and the face met is the body's x face, at 8.  The world normal faces the eye either
    way, to rounding.  Turned 45 degrees about y, the ray through the centre meets a long face, half a unit from the
    axis, at 10 - sqrt(1/2), and the normal is a diagonal."""
    rays = _rays((0, 0, -10), (0, 0, 1))
    h = np.sqrt(0.5)
    b, te, nw = body_pixels(rays, UNIT_BOX, [_body((0, 0, 0), s=(4, 1, 1))])
    assert te[0] == f32(9.5) and tuple(nw[0]) == (0, 0, -1)
    for q, face in (((0, h, 0, h), 1.0), ((0, -h, 0, h), -1.0)):
        b, te, nw = body_pixels(rays, UNIT_BOX, [_body((0, 0, 0), q, (4, 1, 1))])
        assert b[0] == 0 and abs(float(te[0]) - 8.0) < 1e-5
        np.testing.assert_allclose(nw[0], [0, 0, -1], atol=1e-6)
        db = rot(-f32(q[:3]), f32(q[3]), rays[:, 3:6])[0]  # the ray in the body frame runs along the plank
        np.testing.assert_allclose(db, [-face, 0, 0], atol=1e-6)
    q = (0, np.sin(np.pi / 8), 0, np.cos(np.pi / 8))
    b, te, nw = body_pixels(rays, UNIT_BOX, [_body((0, 0, 0), q, (4, 1, 1))])
    assert abs(float(te[0]) - (10.0 - h)) < 1e-5  # the long face, 1/2 from the axis, seen at 45 degrees
    np.testing.assert_allclose(np.abs(nw[0]), [h, 0, h], atol=1e-6)


def test_nearest_body_wins_and_ties_go_to_the_lower_index():
    rays = _rays((0, 0, 0), (0, 0, 1))
    far, near = _body((0, 0, 9)), _body((0, 0, 5))
    assert body_pixels(rays, UNIT_BOX, [far, near])[0][0] == 1
    assert body_pixels(rays, UNIT_BOX, [near, far])[0][0] == 0
    b, te, _ = body_pixels(rays, UNIT_BOX, [far, near, near, far, near])
    assert b[0] == 1 and te[0] == f32(4.5)
    b, te, _ = body_pixels(_rays((0, 0, 5), (0, 0, 1), t0=0.125), UNIT_BOX, [far, near, _body((0.1, 0, 5.1))])
    assert b[0] == 1 and te[0] == f32(0.125)  # two boxes around the eye: both te = t0
    assert body_pixels(rays, UNIT_BOX, [])[0][0] == -1
    assert body_pixels(rays, UNIT_BOX, np.zeros((0, 10), f32))[0][0] == -1
    wide = np.zeros((2, 32), f32)  # the first ten floats of a wider record
    wide[0, :10], wide[1, :10], wide[:, 10:] = far, near, 7.0
    assert body_pixels(rays, UNIT_BOX, wide)[0][0] == 1


# ---------------------------------------------------------------------------- a flat sea
def test_flat_sea_shows_a_floating_box_and_hides_a_sunken_one():
    """Over the plane y = 0: a box that stands on the water is in the picture (status 3, nearer than the water behind
    it, its index and a unit normal in the record, the formula's colour), a box wholly under the plane is met by the
    rays and hidden by the water in front of it, and a box up in the sky is seen against the MISS pixels."""
    tex = _flat()
    w, h, k, steps, refine = 9, 7, 2, 32, 6
    cam = oh.look_at_camera((0.0, 10.0, 0.0), (0.0, 4.0, 30.0), (0, 1, 0), 0.9, w, h, 0.0, 160.0)
    mat, paint = oh.material(), f32([0.9, 0.5, 0.2, 0.7])
    floating, sunken, flying = _body((0, 2, 30), s=(8, 4, 8)), _body((-7, -3, 22), s=(10, 2, 10)), _body((8, 14, 60), s=(14, 10, 14))
    bodies = np.stack([floating, sunken, flying])
    hits, info = restate_camera_bodies(tex, cam, None, w, h, oh.CAMERA_HITS, k, steps, refine, UNIT_BOX, None, bodies)
    rec, b, body = info["rec"], info["b"], info["body"]
    assert hits.dtype == f32 and hits.shape == (w * h, 8)
    assert set(hits[body, 7]) == {0.0, 2.0} and (b == 1).sum() >= 3 and not body[b == 1].any()
    assert (rec[b == 1, 3] == oh.RAY_HIT).all() and (rec[b == 1, 0] < info["te"][b == 1]).all()  # the water is nearer
    assert (rec[b == 2, 3] == oh.RAY_MISS).all() and body[b == 2].all()
    on_water = body & (rec[:, 3] == oh.RAY_HIT)
    assert on_water.sum() >= 3 and (hits[on_water, 0] < rec[on_water, 0]).all() and (b[on_water] == 0).all()
    np.testing.assert_array_equal(hits[body, 3], oh.RAY_BODY)
    np.testing.assert_array_equal(hits[body, 1:3], 0)
    np.testing.assert_allclose(np.linalg.norm(hits[body, 4:7], axis=1), 1.0, atol=1e-6)
    np.testing.assert_array_equal(hits[~body], rec[~body])
    rng, _ = restate_camera_bodies(tex, cam, None, w, h, oh.CAMERA_RANGE, k, steps, refine, UNIT_BOX, None, bodies)
    np.testing.assert_array_equal(rng[body], hits[body, 0])
    np.testing.assert_array_equal(np.isinf(rng), ~body & (rec[:, 3] == oh.RAY_MISS))
    col, _ = restate_camera_bodies(tex, cam, mat, w, h, oh.CAMERA_COLOR, k, steps, refine, UNIT_BOX, paint, bodies)
    col64, _ = restate_camera_bodies(tex, cam, mat, w, h, oh.CAMERA_COLOR, k, steps, refine, UNIT_BOX, paint, bodies,
                                     np.float64)
    assert col.dtype == f32 and col64.dtype == np.float64
    np.testing.assert_array_equal(col[:, 3], hits[:, 3])
    np.testing.assert_allclose(col, col64, rtol=1e-4, atol=1e-6)
    m = mat.astype(np.float64)
    top = body & (hits[:, 5] > 0.99)  # the floating box's upper face: the zenith's light and the sun's
    assert top.any()
    want = paint[:3].astype(np.float64) * (np.float64(paint[3]) * m[29:32] + m[23:26] * max(m[21], 0.0))
    np.testing.assert_allclose(col[top, :3], np.tile(want, (top.sum(), 1)), rtol=1e-5)
    # no bodies: ocean_camera's image
    none, _ = restate_camera_bodies(tex, cam, mat, w, h, oh.CAMERA_COLOR, k, steps, refine, UNIT_BOX, paint, [])
    np.testing.assert_array_equal(none, colours(*shading_inputs(tex, cam, mat, w, h, k, steps, refine), mat, True, f32))
