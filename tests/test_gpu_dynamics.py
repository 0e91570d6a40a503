"""GPU tests of the body dynamics (ocean_body_dynamics / _device / _async, csrc/body.hip k_body_dynamics).  The
entry is restated in numpy fp32 by restate_dynamics of tests/test_dynamics_abi.py over the context's own
read-back textures -- the surface lookup by restate_surface / restate_reference (tests/test_gpu_query.py), the
water's velocity by restate_velocity (tests/test_gpu_velocity.py), the sums by tree_sum -- and the comparison is
bit for bit."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_dynamics_abi import probe_points, restate_dynamics
from test_gpu_body import IDENTITY, PROBES, max_height, random_bodies, random_hull, random_quaternions, reference_lookup
from test_gpu_query import Textures, make_ctx, restate_reference, restate_surface
from test_gpu_velocity import restate_velocity

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
V = oh.F_VELOCITY
LAWS = (oh.DRAG_LINEAR, oh.DRAG_QUADRATIC)
SHAPES = [(64, 1), (64, 4), (128, 2)]
M = 37


def max_speed(vel):
    """An upper bound of the summed velocity's components: sum over the cascades of max |VEL.xyz|."""
    return float(sum(np.abs(vel[c][..., :3]).max() for c in range(vel.shape[0])))


def random_motion(rng, m, vmax):
    """v uniform within +-vmax per component, omega within +-1 rad/s: neither the water nor the hull dominates u."""
    mo = np.empty((m, 6), f32)
    mo[:, :3] = rng.uniform(-vmax, vmax, (m, 3))
    mo[:, 3:] = rng.uniform(-1.0, 1.0, (m, 3))
    return mo


def cases(n, ncasc, size, vmax):
    """(hull, bodies, motion) for every P of PROBES: the hulls and poses of test_gpu_body's restatement test (the
    same generator, seed and draw order, so the same submerged fractions), the motions from a generator of their own."""
    rng, rng_m = np.random.default_rng(1000 * n + ncasc), np.random.default_rng(77 * n + ncasc)
    return [(random_hull(rng, p, size), random_bodies(rng, M, size), random_motion(rng_m, M, vmax)) for p in PROBES]


def surface_inputs(tex, vel, q, ks):
    """{K: (rec, vs)}: the surface query's records at q and Vs at the points they end on."""
    surf, velo = restate_surface(tex, q, ks), restate_velocity(tex, vel, q, ks)
    for k in ks:
        np.testing.assert_array_equal(velo[k][:, 5:7], surf[k][:, 1:3])  # the same p_K
    return {k: (surf[k], velo[k][:, :3]) for k in ks}


def reference_inputs(disp0, vel0, q):
    """(rec, vs) of reference mode: GetWaterHeight's texel of DISP slice 0 and the same texel of VEL slice 0."""
    pick = restate_reference(disp0, q)
    px, py = pick[:, 1].astype(np.int64), pick[:, 2].astype(np.int64)
    return reference_lookup(disp0)(q), vel0[py, px, :3]


@pytest.mark.parametrize("n,ncasc", SHAPES)
def test_dynamics_matches_restatement(n, ncasc):
    """Bit-exact on all 16 floats against the restatement: P in {1, 3, 8, 37, 64, 65, 130} (W = 1, 4, 8, 64 with one,
    two and three chunks), M = 37, K in {0, 4} and reference mode, both laws.  Over all probes of a context at
    least a quarter are partly submerged, 5 % dry and 5 % full."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, V)
    tex, vel = Textures(ctx, cas), ctx.read_all(oh.TEX_VELOCITY)
    size, vmax = max_height(tex.disp), max_speed(vel)
    assert size > 0.0 and vmax > 0.0
    fractions = {0: [], 4: []}
    for hull, bodies, motion in cases(n, ncasc, size, vmax):
        p = len(hull)
        q = probe_points(hull, bodies)
        inputs = surface_inputs(tex, vel, q, (0, 4))
        for k in (0, 4):
            for law in LAWS:
                want, f = restate_dynamics(hull, bodies, motion, law, *inputs[k])
                got = ctx.body_dynamics(hull, bodies, motion, iterations=k, law=law)
                assert got.shape == (M, 16) and np.isfinite(got).all()
                np.testing.assert_array_equal(got, want, err_msg=f"P = {p}, K = {k}, law {law}")
            fractions[k].append(f.ravel())
        rec, vs = reference_inputs(tex.disp[0], vel[0], q)
        for law in LAWS:
            want, _ = restate_dynamics(hull, bodies, motion, law, rec, vs)
            got = ctx.body_dynamics(hull, bodies, motion, iterations=0, mode=oh.QUERY_REFERENCE, law=law)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(got, want, err_msg=f"P = {p}, reference mode, law {law}")
    for k, fs in fractions.items():
        f = np.concatenate(fs)
        partial, dry, full = ((f > 0) & (f < 1)).mean(), (f == 0).mean(), (f == 1).mean()
        print(f"K = {k}: {len(f)} probes, partly submerged {partial:.3f}, dry {dry:.3f}, full {full:.3f}")
        assert partial >= 0.25 and dry >= 0.05 and full >= 0.05
    # the default arguments: surface mode, 4 steps, the linear law
    np.testing.assert_array_equal(ctx.body_dynamics(hull, bodies, motion),
                                  ctx.body_dynamics(hull, bodies, motion, 4, oh.QUERY_SURFACE, oh.DRAG_LINEAR, 0))
    assert np.abs(got[:, 8:14]).max() > 0 and (got[:, 15] > 0).any() and (got[:, 14] > 0).any()
    ctx.close()


@pytest.mark.parametrize("n,ncasc", SHAPES)
def test_first_half_is_the_buoyancy_record(n, ncasc):
    """out[:, :8] equals ocean_body_buoyancy for the same arguments, bit for bit, for every case of the test above."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, V)
    size, vmax = max_height(ctx.read_all(oh.TEX_DISP)), max_speed(ctx.read_all(oh.TEX_VELOCITY))
    for hull, bodies, motion in cases(n, ncasc, size, vmax):
        for kw in (dict(iterations=0), dict(iterations=4), dict(iterations=0, mode=oh.QUERY_REFERENCE)):
            want = ctx.body_buoyancy(hull, bodies, **kw)
            for law in LAWS:
                got = ctx.body_dynamics(hull, bodies, motion, law=law, **kw)
                np.testing.assert_array_equal(got[:, :8], want, err_msg=f"P = {len(hull)}, {kw}, law {law}")
    ctx.close()


def test_one_wet_probe_at_rest_is_the_velocity_query():
    """P = 1, the hull (0, 0, 0, h, 1) held so deep that f = 1 (cy = -h, h = 4 sum_c max |Dy|: eta - bottom =
    eta + 3 h / 2 >= h), the identity pose, unit scale and no motion: g = 1, vb = 0 and u = Vs, so the linear F
    is ocean_query_velocity's Vs at (cx, cz) and the quadratic one f32(m) Vs, with m in out[14].  M = 300: more
    than the 256 one-lane bodies of a workgroup."""
    n, cas, m = 64, O.SCENE_CASCADES[:2], 300
    ctx = make_ctx(n, cas, V)
    size = max_height(ctx.read_all(oh.TEX_DISP))
    rng = np.random.default_rng(6)
    h = f32(4.0 * size)
    hull = f32([[0, 0, 0, h, 1]])
    bodies = random_bodies(rng, m, 0.0)
    bodies[:, 1], bodies[:, 3:7], bodies[:, 7:10] = -h, IDENTITY, 1.0
    motion = np.zeros((m, 6), f32)
    q = np.ascontiguousarray(bodies[:, [0, 2]])
    for k in (0, 4):
        vs = ctx.query_velocity(q, iterations=k)[:, 0:3]
        assert np.abs(vs).max() > 0
        got = ctx.body_dynamics(hull, bodies, motion, iterations=k)
        np.testing.assert_array_equal(got[:, 0], np.ones(m, f32))  # f = 1, g = v' = 1
        np.testing.assert_array_equal(got[:, 8:11], vs)
        np.testing.assert_array_equal(got[:, 15], np.ones(m, f32))
        mag = np.sqrt((vs[:, 0] * vs[:, 0] + vs[:, 1] * vs[:, 1]) + vs[:, 2] * vs[:, 2])
        assert mag.dtype == f32
        np.testing.assert_array_equal(got[:, 14], mag)
        quad = ctx.body_dynamics(hull, bodies, motion, iterations=k, law=oh.DRAG_QUADRATIC)
        np.testing.assert_array_equal(quad[:, 8:11], mag[:, None] * vs)
        np.testing.assert_array_equal(quad[:, 14], mag)
        np.testing.assert_array_equal(quad[:, 15], np.ones(m, f32))
    ctx.close()


def test_known_answers_on_still_water():
    """Before the first ocean_step DISP = VEL = 0: eta = 0, Vs = 0, u = -vb.  The symmetric box of 2 x 2 probes of
    volume 1/4 each (box_hull(2, 2)), at unit scale, held under water (f = 1, g = 1/4, out[0] = 1).
    Translation v = (1, 2, -3), omega = 0: every probe has u = -v.  Linear: F = -v / 4 per probe, sums of power-of-two
    multiples of equal numbers, so sum F = -out[0] v exactly.  Quadratic: m = sqrtf((1 + 4) + 9), s = m / 4 exactly,
    F_i = fl(s (-v_i)) and the four equal terms sum exactly: sum F = -fl(sqrtf(14) v_i), exact but for sqrtf(14)'s own
    rounding.  sum T = sum_j e_j x F_j = (sum_j g_j e_j) x u = out[1..3] x sum F (out[0] = 1); in fp32 each side carries
    per component two products and a difference per probe (3 eps |e| |F|), the products g e (eps) and two levels of
    sums on either side (2 eps each): within 16 eps sum_j |e_j| |F_j|.  The second body is the same box rotated.
    Spin omega = (0, 1, 0), v = 0, scale (4, 1, 4): vb = (e.z, 0, -e.x), F = g (-e.z, 0, e.x), T.y = -g (e.x^2 +
    e.z^2) < 0, a torque opposing the spin; sum F cancels by symmetry to rounding: at most 16 eps sum |F_j|, and with
    |e_xz| = sqrt(2) >= 1 here sum |F_j| <= |out[12]|.  A box lifted clear of the water: out[8..15] = 0."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V, times=())
    hull = oh.OceanContext.box_hull(2, 2)
    rng = np.random.default_rng(12)
    bodies = np.zeros((2, 10), f32)
    bodies[:, :3] = (12.5, -8.0, -40.0)
    bodies[:, 3:7], bodies[:, 7:10] = IDENTITY, 1.0
    bodies[1, 3:7] = random_quaternions(rng, 1)[0]
    v = f32([1.0, 2.0, -3.0])
    motion = np.zeros((2, 6), f32)
    motion[:, :3] = v
    lin = ctx.body_dynamics(hull, bodies, motion)
    np.testing.assert_array_equal(lin[:, 0], np.ones(2, f32))
    np.testing.assert_array_equal(lin[:, 8:11], np.tile(-lin[0, 0] * v, (2, 1)))
    np.testing.assert_array_equal(lin[:, 14], np.full(2, np.sqrt(f32(14.0)), f32))
    np.testing.assert_array_equal(lin[:, 15], np.full(2, 4.0, f32))
    quad = ctx.body_dynamics(hull, bodies, motion, law=oh.DRAG_QUADRATIC)
    np.testing.assert_array_equal(quad[:, 8:11], np.tile(np.sqrt(f32(14.0)) * -v, (2, 1)))
    exact = -np.sqrt(14.0) * v.astype(np.float64)
    assert (np.abs(quad[:, 8:11] - exact) <= 2 * EPS32 * np.abs(exact)).all()
    e_norm = np.sqrt(0.25 ** 2 * 2 + 0.5 ** 2)  # |e| <= |(+-1/4, <= 1/2, +-1/4)| per probe, rotated or not
    for out in (lin, quad):
        f_norm = np.linalg.norm(out[:, 8:11].astype(np.float64), axis=1) / 4  # per probe
        want = np.cross(out[:, 1:4].astype(np.float64), out[:, 8:11].astype(np.float64))
        err = np.abs(out[:, 11:14] - want).max(axis=1)
        print(f"translation: |sum T - out[1..3] x sum F| = {err}, bound {16 * EPS32 * 4 * e_norm * f_norm}")
        assert (err <= 16 * EPS32 * 4 * e_norm * f_norm).all()
    # the spin
    bodies[:, 7:10] = (4.0, 1.0, 4.0)
    motion[:] = (0.0, 0.0, 0.0, 0.0, 1.0, 0.0)
    for law in LAWS:
        out = ctx.body_dynamics(hull, bodies, motion, law=law)
        print(f"spin, law {law}: sum F = {out[:, 8:11].tolist()}, torque y = {out[:, 12].tolist()}")
        assert (out[:, 12] < 0.0).all()
        assert (np.abs(out[:, 8:11]).max(axis=1) <= 16 * EPS32 * np.abs(out[:, 12])).all()
    np.testing.assert_array_equal(ctx.body_dynamics(hull, bodies[:1], motion[:1])[0, 12], f32(-32.0))  # -sum g (1 + 1)
    # lifted clear of the water: every probe dry
    bodies[:, 1] = 1000.0
    motion[:] = (1.0, 2.0, -3.0, 0.5, 1.0, -0.25)
    for law in LAWS:
        out = ctx.body_dynamics(hull, bodies, motion, law=law)
        np.testing.assert_array_equal(out[:, :7], np.zeros((2, 7), f32))
        np.testing.assert_array_equal(out[:, 8:16], np.zeros((2, 8), f32))
    ctx.close()


def test_dynamics_reads_its_own_tile():
    """Two tiles with their own noise: each tile's result equals the restatement over that tile's own DISP, DERIV
    and VEL, and the two differ."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V, tiles=2)
    rng = np.random.default_rng(21)
    got = []
    for tile in range(2):
        tex, vel = Textures(ctx, cas, tile), ctx.read_all(oh.TEX_VELOCITY, tile)
        if tile == 0:
            hull, bodies = random_hull(rng, 37, max_height(tex.disp)), random_bodies(rng, M, max_height(tex.disp))
            motion = random_motion(rng, M, max_speed(vel))
            q = probe_points(hull, bodies)
        rec, vs = surface_inputs(tex, vel, q, (4,))[4]
        for law in LAWS:
            want, _ = restate_dynamics(hull, bodies, motion, law, rec, vs)
            np.testing.assert_array_equal(ctx.body_dynamics(hull, bodies, motion, law=law, tile=tile), want)
        rec, vs = reference_inputs(tex.disp[0], vel[0], q)
        want, _ = restate_dynamics(hull, bodies, motion, oh.DRAG_LINEAR, rec, vs)
        np.testing.assert_array_equal(ctx.body_dynamics(hull, bodies, motion, 0, oh.QUERY_REFERENCE, tile=tile), want)
        got.append(ctx.body_dynamics(hull, bodies, motion, tile=tile))
    assert not np.array_equal(got[0][:, :8], got[1][:, :8]) and not np.array_equal(got[0][:, 8:14], got[1][:, 8:14])
    ctx.close()


def test_dynamics_forms_ordering_and_stats():
    """The device form equals the blocking one; the async request made after step t1, with two more steps queued
    behind it, holds the answer of t1 (a second context gives it) and reads nothing of the caller's after the
    call; *req is NULL after a failure; the launch is kind 2 and named."""
    import torch
    n, cas = 128, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, V, times=()), make_ctx(n, cas, V, times=())
    rng = np.random.default_rng(4)
    hull, bodies = oh.OceanContext.box_hull(5, 3, ny=2), random_bodies(rng, 300, 0.5)
    motion = random_motion(rng, 300, 1.0)
    h, b, mo = hull.copy(), bodies.copy(), motion.copy()
    ctx.set_readback_timing(True)
    ctx.step(times[0])
    rb = ctx.body_dynamics_async(h, b, mo, law=oh.DRAG_QUADRATIC)
    h[:], b[:], mo[:] = 1.0e9, -1.0e9, 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    ms = rb.copy_ms()
    rb.release()
    assert got.shape == (300, 16) and 0.0 < ms < 1000.0
    ref.step(times[0])
    np.testing.assert_array_equal(got, ref.body_dynamics(hull, bodies, motion, law=oh.DRAG_QUADRATIC))
    later = ctx.body_dynamics(hull, bodies, motion, law=oh.DRAG_QUADRATIC)  # the blocking form now: frame t3
    assert not np.array_equal(got[:, 0], later[:, 0]) and not np.array_equal(got[:, 8], later[:, 8])
    ctx.set_readback_timing(False)
    slot = oh.PinnedBuffer(len(bodies) * 64)
    for kw in (dict(), dict(iterations=0), dict(mode=oh.QUERY_REFERENCE, iterations=0)):
        rb = ctx.body_dynamics_async(hull, bodies, motion, buf=slot, **kw)
        np.testing.assert_array_equal(rb.data, ctx.body_dynamics(hull, bodies, motion, **kw))
        rb.release()
    slot.release()
    # a failure hands no request back
    lib, hd, vp = ctx.lib, ctx._h, ctypes.c_void_p
    out = np.zeros((300, 16), f32)
    req = vp(0x1234)
    assert lib.ocean_body_dynamics_async(hd, 0, oh.QUERY_SURFACE, 4, 2, hull.ctypes.data, len(hull), bodies.ctypes.data,
                                         motion.ctypes.data, 300, out.ctypes.data, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert req.value is None and not out.any()
    # the device form, async on the ctx stream
    dev = torch.device("cuda", ctx.device)
    d_h, d_b, d_m = (torch.from_numpy(a.ravel().copy()).to(dev) for a in (hull, bodies, motion))
    d_o = torch.zeros(300 * 16 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.body_dynamics_device(d_h.data_ptr(), len(hull), d_b.data_ptr(), d_m.data_ptr(), 300, d_o.data_ptr(),
                             law=oh.DRAG_QUADRATIC)
    ctx.synchronize()
    np.testing.assert_array_equal(d_o[:4800].cpu().numpy().reshape(300, 16), later)
    assert not d_o[4800:].cpu().numpy().any()
    # counted as kind 2 and named
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)  # (reading resets the counters)
    ctx.body_dynamics(hull, bodies, motion)
    ms, launches = ctx.kernel_stats(2)
    assert launches == 1 and ms > 0.0
    ctx.set_kernel_timing(False)
    assert "k_body_dynamics<32>" in ctx.kernel_name(2)  # 30 probes: 32 lanes per body
    ctx.close()
    ref.close()


def test_dynamics_errors():
    """Every refusal of ocean.h, none of which reaches a kernel (kind 2 counts no launch)."""
    import torch
    cas = O.SCENE_CASCADES[:2]
    hull, bodies, motion = oh.OceanContext.box_hull(2, 2), np.zeros((8, 10), f32), np.zeros((8, 6), f32)
    bodies[:, 3:7], bodies[:, 7:10] = IDENTITY, 1.0
    # a context without the flag
    plain = make_ctx(64, cas, 0, times=(1.0,))
    for call in (plain.body_dynamics, plain.body_dynamics_async):
        with pytest.raises(oh.OceanError) as e:
            call(hull, bodies, motion)
        assert e.value.code == oh.E_UNSUPPORTED
    with pytest.raises(oh.OceanError) as e:  # the argument checks come first
        plain.body_dynamics(hull, bodies, motion, law=2)
    assert e.value.code == oh.E_INVALID_ARG
    plain.close()
    # a velocity context before ocean_init_spectrum
    ctx = oh.OceanContext(64, 2, 1, V)
    for call in (ctx.body_dynamics, ctx.body_dynamics_async):
        with pytest.raises(oh.OceanError) as e:
            call(hull, bodies, motion)
        assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), cas)
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    bad = [dict(tile=1), dict(tile=-1), dict(mode=2), dict(mode=-1), dict(iterations=17), dict(iterations=-1),
           dict(mode=oh.QUERY_REFERENCE, iterations=1), dict(law=2), dict(law=-1)]
    for call in (ctx.body_dynamics, ctx.body_dynamics_async):
        for kw in bad:
            with pytest.raises(oh.OceanError) as e:
                call(hull, bodies, motion, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
        many = oh.BODY_MAX_BODIES + 1
        for h, b in ((np.zeros((0, 5), f32), bodies),                              # probes < 1
                     (np.zeros((oh.BODY_MAX_PROBES + 1, 5), f32), bodies),         # probes > the limit
                     (hull[:1], np.zeros((many, 10), f32)),                        # count > the limit (staged forms)
                     (np.zeros((513, 5), f32), np.zeros((8192, 10), f32))):        # count * probes > 2^22
            with pytest.raises(oh.OceanError) as e:
                call(h, b, np.zeros((len(b), 6), f32))
            assert e.value.code == oh.E_INVALID_ARG, (h.shape, b.shape)
    # nulls and a negative count, through the C entries themselves; *req is reset
    lib, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    out = np.zeros((8, 16), f32)
    hp, bp, mp, op = hull.ctypes.data, bodies.ctypes.data, motion.ctypes.data, out.ctypes.data
    for args in ((None, 4, bp, mp, 8, op), (hp, 4, None, mp, 8, op), (hp, 4, bp, None, 8, op), (hp, 4, bp, mp, 8, None),
                 (hp, 4, bp, mp, -1, op)):
        for name in ("ocean_body_dynamics", "ocean_body_dynamics_device"):
            assert getattr(lib, name)(h, 0, oh.QUERY_SURFACE, 4, 0, *args) == oh.E_INVALID_ARG, (name, args)
        req = vp(0x1234)
        assert lib.ocean_body_dynamics_async(h, 0, oh.QUERY_SURFACE, 4, 0, *args, ctypes.byref(req)) == oh.E_INVALID_ARG
        assert req.value is None
    assert lib.ocean_body_dynamics_async(h, 0, oh.QUERY_SURFACE, 4, 0, hp, 4, bp, mp, 8, op, None) == oh.E_INVALID_ARG
    assert not out.any()
    # count = 0: a no-op in the blocking and device forms, but no request to hand back
    assert ctx.body_dynamics(hull, np.zeros((0, 10), f32), np.zeros((0, 6), f32)).shape == (0, 16)
    with pytest.raises(oh.OceanError) as e:
        ctx.body_dynamics_async(hull, np.zeros((0, 10), f32), np.zeros((0, 6), f32))
    assert e.value.code == oh.E_INVALID_ARG
    dev = torch.device("cuda", ctx.device)
    d_h = torch.zeros(4 * 5 + 1, dtype=torch.float32, device=dev)
    d_b = torch.zeros(8 * 10 + 1, dtype=torch.float32, device=dev)
    d_m = torch.zeros(8 * 6 + 1, dtype=torch.float32, device=dev)
    d_o = torch.zeros(8 * 16 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ph, pb, pm, po = d_h.data_ptr(), d_b.data_ptr(), d_m.data_ptr(), d_o.data_ptr()
    ctx.body_dynamics_device(ph, 4, pb, pm, 0, po)
    # misaligned pointers are refused, not faulted on; count > OCEAN_BODY_MAX_BODIES is not a limit of this form,
    # count * probes (in 64 bits) is
    for a in ((ph + 2, pb, pm, po), (ph, pb + 2, pm, po), (ph, pb, pm + 2, po), (ph, pb, pm, po + 4)):
        with pytest.raises(oh.OceanError) as e:
            ctx.body_dynamics_device(a[0], 4, a[1], a[2], 8, a[3])
        assert e.value.code == oh.E_INVALID_ARG, a
    for probes, count in ((1, oh.BODY_MAX_SAMPLES + 1), (4096, 1 << 20), (4096, 1025)):
        with pytest.raises(oh.OceanError) as e:
            ctx.body_dynamics_device(ph, probes, pb, pm, count, po)
        assert e.value.code == oh.E_INVALID_ARG, (probes, count)
    ctx.synchronize()
    assert ctx.kernel_stats(2)[1] == 0  # none of the above reached a kernel
    ctx.set_kernel_timing(False)
    # the limits themselves are served by the staged forms (592 KiB of inputs, 512 KiB of records): body b equals
    # body b alone
    rng = np.random.default_rng(2)
    big_hull, big = random_hull(rng, 512, 2.0), random_bodies(rng, oh.BODY_MAX_BODIES, 1.0)
    big_motion = random_motion(rng, oh.BODY_MAX_BODIES, 1.0)
    rb = ctx.body_dynamics_async(big_hull, big, big_motion)
    got = rb.data.copy()
    rb.release()
    assert got.shape == (oh.BODY_MAX_BODIES, 16) and np.isfinite(got).all()
    pick = [0, 1, 4097, 8191]
    np.testing.assert_array_equal(got[pick], ctx.body_dynamics(big_hull, big[pick], big_motion[pick]))
    ctx.close()
