"""CPU tests of the body-step entries (ocean_body_step, _device, _async; include/ocean/ocean.h): what can be checked
without a GPU -- the symbols, the constants, the validation that needs no context -- and restate_step, the numpy fp32
statement of one substep that tests/test_gpu_step.py compares the kernel with bit for bit, itself pinned here by
known answers: free fall, a wrench integrated by hand, the reference's BuoyantObject.FixedUpdate written
independently in float64, and the quaternion's norm."""
import ctypes

import numpy as np

import ocean_hip as oh
from test_dynamics_abi import restate_dynamics
from test_gpu_body import cross

STEP_SYMBOLS = ("ocean_body_step", "ocean_body_step_device", "ocean_body_step_async")
f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


def rot(u, w, a):
    """rot(u, w, a) of ocean.h: t = 2 (u x a), (a + w t) + (u x t)."""
    t = tuple(f32(2.0) * c for c in cross(u, a))
    ut = cross(u, t)
    return tuple((a[i] + w * t[i]) + ut[i] for i in range(3))


def restate_step(rec, state, props, step):
    """One substep of ocean_body_step in numpy fp32, in ocean.h's operation order.  rec float32[M][16]: the dynamics
    record at `state` (restate_dynamics, or the kernel's own); state float32[M][>= 16] = (c, q, s, v, o); props
    float32[M][4]; step float32[8].  Returns the state after the substep, float32[M][16]."""
    rec = np.asarray(rec, f32).reshape(-1, 16)
    st = np.asarray(state, f32)[:, :16]
    pr = np.asarray(props, f32).reshape(-1, 4)
    h, g, B, kd, kt, la, aa = (f32(x) for x in np.asarray(step, f32).reshape(-1)[:7])
    c, u, qw = (st[:, 0], st[:, 1], st[:, 2]), (st[:, 3], st[:, 4], st[:, 5]), st[:, 6]
    v, o = (st[:, 10], st[:, 11], st[:, 12]), (st[:, 13], st[:, 14], st[:, 15])
    im, j = pr[:, 0], (pr[:, 1], pr[:, 2], pr[:, 3])
    acc = (im * (kd * rec[:, 8]), im * (B * rec[:, 0] + kd * rec[:, 9]) - g, im * (kd * rec[:, 10]))
    tau = (kt * rec[:, 11] - B * rec[:, 3], kt * rec[:, 12], kt * rec[:, 13] + B * rec[:, 1])
    tb = rot(tuple(-x for x in u), qw, tau)
    alp = rot(u, qw, tuple(j[i] * tb[i] for i in range(3)))
    wet = rec[:, 15] > f32(0.0)
    v1 = [v[i] + h * acc[i] for i in range(3)]
    o1 = [o[i] + h * alp[i] for i in range(3)]
    v1 = [np.where(wet, v1[i] - (v[i] * la) * h, v1[i]) for i in range(3)]
    o1 = [np.where(wet, o1[i] - (o[i] * aa) * h, o1[i]) for i in range(3)]
    hh = f32(0.5) * h
    oxu = cross(o1, u)
    n = [u[i] + hh * (qw * o1[i] + oxu[i]) for i in range(3)]
    nw = qw - hh * ((o1[0] * u[0] + o1[1] * u[1]) + o1[2] * u[2])
    ln = np.sqrt(((n[0] * n[0] + n[1] * n[1]) + n[2] * n[2]) + nw * nw)
    out = st.copy()
    for i in range(3):
        out[:, i] = c[i] + h * v1[i]
        out[:, 3 + i] = n[i] / ln
        out[:, 10 + i] = v1[i]
        out[:, 13 + i] = o1[i]
    out[:, 6] = nw / ln
    assert out.dtype == f32 and ln.dtype == f32 and acc[1].dtype == f32
    return out


def _args(ctx=None, mode=oh.QUERY_SURFACE, iterations=4, law=oh.DRAG_LINEAR, substeps=1, step="ok", hull="ok", probes=1,
          props="ok", state="ok", count=2, out="ok", keep=[]):
    """The thirteen arguments of ocean_body_step with valid defaults; "ok" stands for a buffer of the right size."""
    bufs = dict(step=oh.step_params(0.02), hull=np.zeros((1, 5), f32), props=np.zeros((2, 4), f32),
                state=np.zeros((2, 32), f32), out=np.zeros((2, 32), f32))
    keep.append(bufs)  # (the buffers outlive the call)
    given = dict(step=step, hull=hull, props=props, state=state, out=out)
    p = {}
    for k, a in given.items():
        if isinstance(a, np.ndarray):
            keep.append(a)
        p[k] = bufs[k].ctypes.data if isinstance(a, str) else (None if a is None else a.ctypes.data)
    return (ctx, 0, mode, iterations, law, substeps, p["step"], p["hull"], probes, p["props"], p["state"], count, p["out"])


def test_step_symbols_exported():
    L = oh.load_library()
    for s in STEP_SYMBOLS:
        assert s in oh.EXPORTED_SYMBOLS
        assert hasattr(L, s)
    assert (oh.BODY_STEP_FLOATS, oh.BODY_MAX_SUBSTEPS, oh.BODY_STEP_MAX_SAMPLES) == (8, 64, 1 << 24)
    assert L.ocean_abi_version() == 4  # added within version 4 (ocean.h version history)
    for name in ("body_step", "body_step_async", "body_step_device", "body_state"):
        assert callable(getattr(oh.OceanContext, name)), name
    assert callable(oh.WaterBody.StepBodies)


def test_step_params_layout():
    """(h, g, B, kd, kt, la, aa, 0); B defaults to g * density, the reference's buoyant acceleration per volume."""
    p = oh.step_params(0.02)
    assert p.dtype == f32 and p.shape == (8,)
    np.testing.assert_array_equal(p, f32([0.02, 9.81, 9.81, 0, 0, 0, 0, 0]))
    p = oh.step_params(0.01, g=10.0, density=2.0, drag=3.0, drag_torque=4.0, linear_damping=5.0, angular_damping=6.0)
    np.testing.assert_array_equal(p, f32([0.01, 10, 20, 3, 4, 5, 6, 0]))
    assert oh.step_params(0.01, buoyancy=7.0)[2] == f32(7.0)
    s = oh.OceanContext.body_state(np.arange(20, dtype=f32).reshape(2, 10), np.ones((2, 6), f32))
    assert s.shape == (2, 32) and not s[:, 16:].any() and (s[:, 10:16] == 1).all() and s[1, 9] == 19


def test_step_null_context_is_invalid_arg():
    """Validated before any device call: no GPU is touched, here there is none."""
    L = oh.load_library()
    for name in ("ocean_body_step", "ocean_body_step_device"):
        L.ocean_host_alloc(0, None)  # (leaves another message behind)
        assert getattr(L, name)(*_args()) == oh.E_INVALID_ARG, name
        assert b"context" in L.ocean_last_error(), name
    req = ctypes.c_void_p(0x1234)
    L.ocean_host_alloc(0, None)
    assert L.ocean_body_step_async(*_args(), ctypes.byref(req)) == oh.E_INVALID_ARG
    assert b"context" in L.ocean_last_error()
    assert req.value is None  # no request handed back
    assert L.ocean_body_step_async(*_args(), None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()


def test_step_argument_checks_that_need_no_context():
    """The entry's own arguments are checked before the context is looked at, so every one of them can be seen
    failing here, by its message: a null step, props or state, an unknown law, a step value that is not finite,
    substeps outside [1, 64], count * probes * substeps > 2^24 in 64 bits; then the bodies' checks, which begin with
    the context.  Every form, and *req is NULL after each."""
    L = oh.load_library()
    nan_step, inf_step = oh.step_params(0.02), oh.step_params(0.02)
    nan_step[3], inf_step[0] = np.nan, np.inf
    bad = [(dict(step=None), b"null step"), (dict(props=None), b"null step"), (dict(state=None), b"null step"),
           (dict(law=2), b"law"), (dict(law=-1), b"law"),
           (dict(step=nan_step), b"step[3]"), (dict(step=inf_step), b"step[0]"),
           (dict(substeps=0), b"substeps"), (dict(substeps=oh.BODY_MAX_SUBSTEPS + 1), b"substeps"), (dict(substeps=-3), b"substeps"),
           # 2^13 * 2^9 = 2^22 samples, which the bodies allow, times 8 substeps
           (dict(count=8192, probes=512, substeps=8), b"OCEAN_BODY_STEP_MAX_SAMPLES"),
           (dict(count=1 << 20, probes=4096, substeps=64), b"OCEAN_BODY_STEP_MAX_SAMPLES"),  # 2^38: 64-bit
           # what passes them reaches the bodies' checks
           (dict(count=8192, probes=512, substeps=4), b"context"), (dict(substeps=oh.BODY_MAX_SUBSTEPS), b"context"),
           (dict(hull=None), b"context"), (dict(out=None), b"context"), (dict(count=-1), b"context")]
    for kw, word in bad:
        for name in ("ocean_body_step", "ocean_body_step_device"):
            L.ocean_host_alloc(0, None)
            assert getattr(L, name)(*_args(**kw)) == oh.E_INVALID_ARG, (name, kw)
            assert word in L.ocean_last_error(), (name, kw, L.ocean_last_error())
        req = ctypes.c_void_p(0x1234)
        L.ocean_host_alloc(0, None)
        assert L.ocean_body_step_async(*_args(**kw), ctypes.byref(req)) == oh.E_INVALID_ARG, kw
        assert word in L.ocean_last_error(), (kw, L.ocean_last_error())
        assert req.value is None


def _state(c=(0, 0, 0), q=(0, 0, 0, 1), s=(1, 1, 1), v=(0, 0, 0), o=(0, 0, 0)):
    st = np.zeros((1, 32), f32)
    st[0, :16] = list(c) + list(q) + list(s) + list(v) + list(o)
    return st


def test_restatement_free_fall():
    """No wet probe (rec = 0), la = aa = 0, ten substeps: acc = (0, im * (B * 0 + kd * 0) - g, 0) = (0, 0 - g, 0), so
    v.y follows the fp32 loop v = v + h * (0 - g) and c.y the loop c = c + h * v, written out here; x and z do not move;
    with o = 0 the quaternion does not change by a bit (n = u + hh * 0, len = 1 for both quaternions used, whose
    squares sum to 1 exactly)."""
    step = oh.step_params(1.0 / 60.0, g=9.81, drag=3.0, drag_torque=2.0)
    h, g = step[0], step[1]
    props = f32([[0.25, 1.0, 2.0, 3.0]])
    for q in ((0, 0, 0, 1), (0.5, 0.5, 0.5, 0.5)):
        st = _state(c=(3.0, 100.0, -7.0), q=q, s=(1.0, 2.0, 0.5), v=(0.0, 1.5, 0.0))
        vy, cy = f32(1.5), f32(100.0)
        for _ in range(10):
            st = restate_step(np.zeros((1, 16), f32), st, props, step)
            vy = vy + h * (f32(0.0) - g)
            cy = cy + h * vy
            assert vy.dtype == f32 and cy.dtype == f32
        assert st[0, 11] == vy and st[0, 1] == cy
        assert vy < f32(0.0) and cy != f32(100.0)
        np.testing.assert_array_equal(st[0, [0, 2]], f32([3.0, -7.0]))
        np.testing.assert_array_equal(st[0, 3:7], f32(q))
        np.testing.assert_array_equal(st[0, 7:10], f32([1.0, 2.0, 0.5]))
        np.testing.assert_array_equal(st[0, [10, 12, 13, 14, 15]], np.zeros(5, f32))


def test_restatement_against_a_hand_computed_wrench():
    """q = (1/2, 1/2, 1/2, 1/2): the rotation R by 120 degrees about (1, 1, 1), R (a, b, c) = (c, a, b), exact in fp32.
    step = (h 1/2, g 10, B 4, kd 2, kt 1/2, la 1/4, aa 1/2); im = 1/2, j = (1, 2, 4).
    rec: V = 3/2, first moments (1/2, -, -1/4), sum F = (1, 2, -1), sum T = (4, -2, 6), two wet probes.
    acc = (1/2 (2 * 1), 1/2 (4 * 3/2 + 2 * 2) - 10, 1/2 (2 * -1)) = (1, -5, -1).
    tau = (1/2 * 4 - 4 * -1/4, 1/2 * -2, 1/2 * 6 + 4 * 1/2) = (3, -1, 5); tb = R^-1 tau = (-1, 5, 3);
    j tb = (-1, 10, 12); alp = R (j tb) = (12, -1, 10).
    v = (2, -1, 4): v + h acc = (5/2, -7/2, 7/2), less (v la) h = (1/4, -1/8, 1/2): v' = (9/4, -27/8, 3).
    o = (1/2, 1, -1/2): o + h alp = (13/2, 1/2, 9/2), less (o aa) h = (1/8, 1/4, -1/8): o' = (51/8, 1/4, 37/8).
    c = (1, 2, 3): c' = c + h v' = (17/8, 5/16, 9/2).
    qw o' + o' x u = (51/16, 1/8, 37/16) + (-35/16, -7/8, 49/16) = (1, -3/4, 43/8); n = u + 1/4 (..) = (3/4, 5/16, 59/32);
    o'.u = 45/8, nw = 1/2 - 45/32 = -29/32; len^2 = 4.880859375, every operation so far exact in fp32.  sqrtf and the four
    divisions round once each: q' within 2 eps of the float64 quotient.  Dry (rec[15] = 0): no damping."""
    step = f32([0.5, 10.0, 4.0, 2.0, 0.5, 0.25, 0.5, 0.0])
    props = f32([[0.5, 1.0, 2.0, 4.0]])
    st = _state(c=(1, 2, 3), q=(0.5, 0.5, 0.5, 0.5), s=(2, 3, 4), v=(2, -1, 4), o=(0.5, 1, -0.5))
    rec = f32([[1.5, 0.5, 9.0, -0.25, 9.0, 9.0, 9.0, 9.0, 1.0, 2.0, -1.0, 4.0, -2.0, 6.0, 3.0, 2.0]])
    np.testing.assert_array_equal(np.stack(rot((f32(0.5),) * 3, f32(0.5), (f32(1.0), f32(2.0), f32(3.0)))), f32([3, 1, 2]))
    out = restate_step(rec, st, props, step)
    assert out.dtype == f32 and out.shape == (1, 16)
    np.testing.assert_array_equal(out[0, :3], f32([2.125, 0.3125, 4.5]))
    np.testing.assert_array_equal(out[0, 7:10], f32([2, 3, 4]))
    np.testing.assert_array_equal(out[0, 10:13], f32([2.25, -3.375, 3.0]))
    np.testing.assert_array_equal(out[0, 13:16], f32([6.375, 0.25, 4.625]))
    want_q = np.float64([0.75, 0.3125, 1.84375, -0.90625]) / np.sqrt(np.float64(4.880859375))
    assert (np.abs(out[0, 3:7] - want_q) <= 2 * EPS32 * np.abs(want_q)).all()
    rec[0, 15] = 0.0
    dry = restate_step(rec, st, props, step)
    np.testing.assert_array_equal(dry[0, 10:13], f32([2.5, -3.5, 3.5]))
    np.testing.assert_array_equal(dry[0, 13:16], f32([6.5, 0.5, 4.5]))
    np.testing.assert_array_equal(dry[0, :3], f32([2.25, 0.25, 4.75]))
    # zero props: no force or torque moves the body; gravity's -g is an acceleration and still does
    still = restate_step(rec, st, np.zeros((1, 4), f32), step)
    np.testing.assert_array_equal(still[0, 10:16], f32([2, -6, 4, 0.5, 1, -0.5]))


def fixed_update_f64(y, v, o, scale, eta, dt, g, density, drag, angular_drag):
    """What the reference's BuoyantObject does in one fixed update, as behaviour, in float64: the submerged height
    eta - y over the box's height gives the submerged share of the volume sx sy sz; while it is positive the body
    gets the upward acceleration g density V and loses the shares drag dt of its velocity and angularDrag dt of its
    angular velocity; gravity always; then semi-implicit Euler: v += a dt, x += v dt."""
    a = -g
    dv, do = np.zeros(3), np.zeros(3)
    submerged = max(0.0, eta - y)
    if submerged > 0.0:
        volume = min(max(submerged / scale[1], 0.0), 1.0) * (scale[0] * scale[1] * scale[2])
        a += g * (density * volume)
        dv, do = -v * drag * dt, -o * angular_drag * dt
    v = v + dv + np.array([0.0, a * dt, 0.0])
    return v, o + do


FIXED_UPDATE_TOL = 4 * 2.3e-6  # four times the largest deviation measured between the two restatements (below)


def test_restatement_is_the_reference_fixed_update():
    """The reference's physics path as one entry: the one-probe hull (0, 0.5, 0, 1, 1) in reference mode, im = 1,
    kd = kt = 0, B = g density, la = drag, aa = angularDrag.  The probe's cell then is the box: bottom = c.y, h' = sy,
    v' = sx sy sz.  200 substeps of 1/50 s over synthetic water heights (a swell of 0.8 m and 7 s with a chop on it),
    a box of (1, 0.5, 2) m dropped from 1 m with a horizontal velocity and a yaw rate (a rotation about y leaves the
    probe at (0, sy / 2, 0) exactly): it dives, bobs up and settles riding the swell, wet and dry in turns at first.
    fp32 restatement (restate_dynamics for the record, restate_step behind it) against fixed_update_f64: neither is the
    code under test.  Measured here on the CPU over the 200 substeps: largest |difference| 4.3e-7 in position (m),
    2.3e-6 in velocity (m/s), 9.3e-8 in angular velocity (rad/s); the bound is four times the largest."""
    dt, g, density, drag, adrag = 0.02, 9.81, 1.5, 2.0, 1.0
    scale = (1.0, 0.5, 2.0)
    hull = f32([[0, 0.5, 0, 1, 1]])
    props = f32([[1.0, 1.0, 1.0, 1.0]])
    step = oh.step_params(dt, g=g, density=density, linear_damping=drag, angular_damping=adrag)
    st = _state(c=(0.0, 1.0, 0.0), s=scale, v=(0.5, 0.0, -0.25), o=(0.0, 0.75, 0.0))
    x, v, o = np.float64([0.0, 1.0, 0.0]), np.float64([0.5, 0.0, -0.25]), np.float64([0.0, 0.75, 0.0])
    worst = np.zeros(3)
    wet_steps = 0
    for k in range(200):
        t = k * dt
        eta = 0.8 * np.sin(2 * np.pi * t / 7.0) + 0.05 * np.sin(2 * np.pi * t / 0.9)
        probe = f32([[eta, 0, 0, 0, 0, 1, 0, 0]])  # the reference-mode record: eta, n = (0, 1, 0), r = 0
        rec, f = restate_dynamics(hull, st[:, :10], st[:, 10:16], oh.DRAG_LINEAR, probe, np.zeros((1, 3), f32))
        wet_steps += int(rec[0, 15] > 0)
        st = restate_step(rec, st, props, step)
        v, o = fixed_update_f64(x[1], v, o, scale, float(f32(eta)), dt, g, density, drag, adrag)
        x = x + v * dt
        worst = np.maximum(worst, [np.abs(st[0, :3] - x).max(), np.abs(st[0, 10:13] - v).max(), np.abs(st[0, 13:16] - o).max()])
    print(f"fixed update, 200 substeps: wet in {wet_steps}; largest |fp32 - float64| position {worst[0]:.3g}, "
          f"velocity {worst[1]:.3g}, angular velocity {worst[2]:.3g}")
    assert 20 <= wet_steps < 200  # both branches were taken
    assert abs(st[0, 1]) < 2.0 and abs(x[1]) < 2.0  # it floats
    assert worst.max() <= FIXED_UPDATE_TOL
    # the probe stayed where the reference looks: yaw alone, so d = (0, sy / 2, 0) and no torque
    assert st[0, 3] == 0 and st[0, 5] == 0 and st[0, 4] != 0
    assert st[0, 13] == 0 and st[0, 15] == 0


def test_quaternion_stays_unit():
    """|q'| = 1 within 2 ulp of 1 after 1000 substeps at |o| <= 1 rad/s.  len^2 carries four squares and three sums,
    sqrtf halves its relative error and adds a rounding, each quotient adds one: every component is within 4 u of
    n_i / |n| (u = eps / 2), and so is the norm: 4 u = 2 eps = 2 ulp of 1.  The error does not accumulate, since each
    substep normalises anew."""
    rng = np.random.default_rng(8)
    m = 64
    o = rng.standard_normal((m, 3))
    o = o / np.linalg.norm(o, axis=1, keepdims=True) * rng.uniform(0.1, 1.0, (m, 1))
    q = rng.standard_normal((m, 4))
    st = np.zeros((m, 32), f32)
    st[:, 3:7] = q / np.linalg.norm(q, axis=1, keepdims=True)
    st[:, 7:10], st[:, 13:16] = 1.0, o
    step = oh.step_params(1.0 / 50.0)
    props, rec = np.ones((m, 4), f32), np.zeros((m, 16), f32)
    first = st[:, 3:7].copy()
    worst = 0.0
    for _ in range(1000):
        st = restate_step(rec, st, props, step)
        worst = max(worst, float(np.abs(np.linalg.norm(st[:, 3:7].astype(np.float64), axis=1) - 1.0).max()))
    print(f"largest ||q| - 1| over 1000 substeps of {m} bodies: {worst:.3g} = {worst / EPS32:.2f} eps")
    assert worst <= 2 * EPS32
    np.testing.assert_array_equal(st[:, 13:16], o.astype(f32))  # no torque: the spin is kept
    # 20 s at 0.1 .. 1 rad/s: the bodies have turned by |o| T about o.  q' conj(q) has the scalar part cos(|o| T / 2);
    # a substep turns by 2 atan(|o| h / 2), short of |o| h by a share (|o| h)^2 / 12 <= 3.4e-5: over at most 20 rad that
    # is 7e-4 rad, 3.4e-4 in the cosine of the half angle
    turn = np.linalg.norm(o, axis=1) * 1000 * float(step[0])
    got = (st[:, 3:7].astype(np.float64) * first).sum(axis=1)
    assert turn.max() > 6.3 and np.abs(got - np.cos(turn / 2)).max() <= 5e-4
