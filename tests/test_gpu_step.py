"""GPU tests of the body steps (ocean_body_step / _device / _async, csrc/body.hip k_body_step).  One substep is its
parts: the record of ocean_body_dynamics, which tests/test_gpu_dynamics.py holds to its restatement, and restate_step
of tests/test_step_abi.py behind it, bit for bit; S substeps are S such calls chained."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_dynamics_abi import probe_points, restate_dynamics
from test_gpu_body import IDENTITY, max_height, random_bodies, random_hull
from test_gpu_dynamics import LAWS, M, SHAPES, cases, max_speed, random_motion, surface_inputs
from test_gpu_query import Textures, make_ctx
from test_step_abi import restate_step

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
V = oh.F_VELOCITY
# h, g, B, kd, kt, la, aa: every term of the substep takes part
STEP = oh.step_params(1.0 / 60.0, g=9.81, buoyancy=12.5, drag=0.5, drag_torque=0.25, linear_damping=0.75,
                      angular_damping=0.375)
MODES = (dict(iterations=0), dict(iterations=4), dict(iterations=0, mode=oh.QUERY_REFERENCE))


def random_props(rng, m, hull):
    """Inverse mass and inverse principal moments, all different: 0.05 .. 1 over the largest volume a body of this
    hull can displace (scales up to 3 per axis), so that the accelerations stay of the order of g and B and the
    explicit drag terms stay stable over the substeps of a test: the states compared are finite numbers."""
    return (rng.uniform(0.05, 1.0, (m, 4)) / (27.0 * float(np.asarray(hull)[:, 4].sum()))).astype(f32)


def state_of(bodies, motion):
    """float32[M][32] with a pattern in the sixteen floats the entry ignores on input."""
    s = oh.OceanContext.body_state(bodies, motion)
    s[:, 16:] = np.arange(16, dtype=f32) - 7.5
    return s


def parts(ctx, hull, state, props, step, **kw):
    """One substep from its parts: (the state restate_step gives behind ocean_body_dynamics' record, that record)."""
    rec = ctx.body_dynamics(hull, state[:, :10].copy(), state[:, 10:16].copy(), **kw)
    return np.concatenate([restate_step(rec, state, props, step), rec], axis=1)


@pytest.mark.parametrize("n,ncasc", SHAPES)
def test_one_substep_equals_its_parts(n, ncasc):
    """P in {1, 3, 8, 37, 64, 65, 130}, M = 37, K in {0, 4} and reference mode, both laws: out[:, 16:] is
    ocean_body_dynamics' record and out[:, :16] restate_step of it, bit for bit.  Over all probes of a context at least
    a quarter are partly submerged and 5 % dry (the hulls, poses and motions of tests/test_gpu_dynamics.py)."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, V)
    tex, vel = Textures(ctx, cas), ctx.read_all(oh.TEX_VELOCITY)
    size, vmax = max_height(tex.disp), max_speed(vel)
    rng = np.random.default_rng(5 * n + ncasc)
    fractions = []
    moved = 0.0
    for hull, bodies, motion in cases(n, ncasc, size, vmax):
        state, props = state_of(bodies, motion), random_props(rng, M, hull)
        for kw in MODES:
            for law in LAWS:
                got = ctx.body_step(hull, state, props, STEP, 1, law=law, **kw)
                assert got.shape == (M, 32) and np.isfinite(got).all()
                want = parts(ctx, hull, state, props, STEP, law=law, **kw)
                np.testing.assert_array_equal(got[:, 16:], want[:, 16:], err_msg=f"record: P = {len(hull)}, {kw}, law {law}")
                np.testing.assert_array_equal(got[:, :16], want[:, :16], err_msg=f"state: P = {len(hull)}, {kw}, law {law}")
                moved = max(moved, float(np.abs(got[:, 13:16] - state[:, 13:16]).max()))
        _, f = restate_dynamics(hull, bodies, motion, oh.DRAG_LINEAR, *surface_inputs(tex, vel, probe_points(hull, bodies), (4,))[4])
        fractions.append(f.ravel())
    f = np.concatenate(fractions)
    partial, dry = ((f > 0) & (f < 1)).mean(), (f == 0).mean()
    print(f"{len(f)} probes, partly submerged {partial:.3f}, dry {dry:.3f}")
    assert partial >= 0.25 and dry >= 0.05
    assert moved > 0.0  # torques reached the angular velocity
    # the default arguments: one substep, surface mode, 4 steps, the linear law
    np.testing.assert_array_equal(ctx.body_step(hull, state, props, STEP),
                                  ctx.body_step(hull, state, props, STEP, 1, 4, oh.QUERY_SURFACE, oh.DRAG_LINEAR, 0))
    ctx.close()


@pytest.mark.parametrize("n,ncasc", SHAPES)
def test_substeps_are_a_loop(n, ncasc):
    """S = 5 in one call equals five chained S = 1 calls, bit for bit on all 32 floats: the state, and the record of
    the fifth call (taken at the state the fifth substep started from)."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, V)
    size, vmax = max_height(ctx.read_all(oh.TEX_DISP)), max_speed(ctx.read_all(oh.TEX_VELOCITY))
    rng = np.random.default_rng(11 * n + ncasc)
    for p, kw, law in ((8, MODES[1], oh.DRAG_QUADRATIC), (37, MODES[0], oh.DRAG_LINEAR), (65, MODES[2], oh.DRAG_QUADRATIC)):
        hull, bodies, motion = random_hull(rng, p, size), random_bodies(rng, M, size), random_motion(rng, M, vmax)
        state, props = state_of(bodies, motion), random_props(rng, M, hull)
        once = ctx.body_step(hull, state, props, STEP, 5, law=law, **kw)
        chained = state
        for _ in range(5):
            before = chained
            chained = ctx.body_step(hull, chained, props, STEP, 1, law=law, **kw)
        assert np.isfinite(once).all()
        np.testing.assert_array_equal(once, chained, err_msg=f"P = {p}, {kw}, law {law}")
        np.testing.assert_array_equal(once, parts(ctx, hull, before, props, STEP, law=law, **kw))
        assert not np.array_equal(once[:, 16:], ctx.body_step(hull, state, props, STEP, 1, law=law, **kw)[:, 16:])
    ctx.close()


def test_in_place_on_the_device():
    """ocean_body_step_device with out == state over a device buffer equals the blocking form; a second in-place call
    equals the blocking form with the substeps doubled.  Nothing is written outside the records."""
    import torch
    n, cas, p, s = 64, O.SCENE_CASCADES[:2], 37, 3
    ctx = make_ctx(n, cas, V)
    size, vmax = max_height(ctx.read_all(oh.TEX_DISP)), max_speed(ctx.read_all(oh.TEX_VELOCITY))
    rng = np.random.default_rng(31)
    hull, bodies, motion = random_hull(rng, p, size), random_bodies(rng, M, size), random_motion(rng, M, vmax)
    state, props = state_of(bodies, motion), random_props(rng, M, hull)
    dev = torch.device("cuda", ctx.device)
    d_h, d_p = (torch.from_numpy(a.ravel().copy()).to(dev) for a in (hull, props))
    d_s = torch.full((M * 32 + 8,), -3.0, dtype=torch.float32, device=dev)
    d_s[:M * 32] = torch.from_numpy(state.ravel().copy()).to(dev)
    torch.cuda.synchronize()
    for calls in (1, 2):
        ctx.body_step_device(d_h.data_ptr(), p, d_p.data_ptr(), d_s.data_ptr(), M, d_s.data_ptr(), STEP, s,
                             law=oh.DRAG_QUADRATIC)
        ctx.synchronize()
        got = d_s.cpu().numpy()
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got[:M * 32].reshape(M, 32),
                                      ctx.body_step(hull, state, props, STEP, calls * s, law=oh.DRAG_QUADRATIC))
        np.testing.assert_array_equal(got[M * 32:], np.full(8, -3.0, f32))
    # out of place: the state is left as it was
    d_o = torch.zeros(M * 32, dtype=torch.float32, device=dev)
    before = d_s.cpu().numpy()
    torch.cuda.synchronize()
    ctx.body_step_device(d_h.data_ptr(), p, d_p.data_ptr(), d_s.data_ptr(), M, d_o.data_ptr(), STEP, s, law=oh.DRAG_QUADRATIC)
    ctx.synchronize()
    np.testing.assert_array_equal(d_s.cpu().numpy(), before)
    np.testing.assert_array_equal(d_o.cpu().numpy().reshape(M, 32),
                                  ctx.body_step(hull, state, props, STEP, 3 * s, law=oh.DRAG_QUADRATIC))
    ctx.close()


@pytest.mark.parametrize("p,m", [(1, 300), (130, 5)])
def test_more_than_a_workgroup(p, m):
    """P = 1, M = 300: 256 one-lane bodies per workgroup, so two workgroups, the second partly filled.  P = 130, M = 5:
    a wave per body and three trips, four bodies per workgroup.  One substep from its parts, three as a chain."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V)
    size, vmax = max_height(ctx.read_all(oh.TEX_DISP)), max_speed(ctx.read_all(oh.TEX_VELOCITY))
    rng = np.random.default_rng(100 * p + m)
    hull, bodies, motion = random_hull(rng, p, size), random_bodies(rng, m, size), random_motion(rng, m, vmax)
    state, props = state_of(bodies, motion), random_props(rng, m, hull)
    for law in LAWS:
        chained = state
        for _ in range(3):
            got = ctx.body_step(hull, chained, props, STEP, 1, law=law)
            np.testing.assert_array_equal(got, parts(ctx, hull, chained, props, STEP, law=law))
            chained = got
        np.testing.assert_array_equal(ctx.body_step(hull, state, props, STEP, 3, law=law), chained)
    assert (chained[:, 31] > 0).any() and np.isfinite(chained).all()
    ctx.close()


def test_flat_water_scenario():
    """A velocity context before its first ocean_step: DISP = VEL = 0, which ocean.h guarantees valid, so the water
    is known: eta = 0, n = (0, 1, 0), r = 0, Vs = 0 at every probe.  An upright unit box of 2 x 2 probes of half the
    water's density (im B = 2 g: it floats half submerged), dropped from just above the surface, linear drag against
    the water and the reference's damping: 8 calls of 64 substeps of 1/240 s equal 512 substeps of the fp32
    restatement (restate_dynamics over that water, restate_step behind it) bit for bit, wet count, submerged volume
    and the sign of v.y at the end included.  A second body, rolled and with a spin, rides along."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V, times=())
    hull = oh.OceanContext.box_hull(2, 2)
    bodies = np.zeros((2, 10), f32)
    bodies[:, :3], bodies[:, 3:7], bodies[:, 7:10] = (3.0, 0.55, -2.0), IDENTITY, 1.0
    bodies[1, 3:7] = (0.28, 0.0, 0.0, 0.96)
    motion = np.zeros((2, 6), f32)
    motion[1] = (0.25, 0.0, -0.5, 0.0, 0.5, 0.25)
    props = f32([[1.0, 6.0, 6.0, 6.0], [1.0, 6.0, 3.0, 2.0]])
    step = oh.step_params(1.0 / 240.0, g=9.81, buoyancy=2 * 9.81, drag=2.0, drag_torque=2.0, linear_damping=1.0,
                          angular_damping=0.5)
    got = want = state_of(bodies, motion)
    water = np.zeros((2 * len(hull), 8), f32)
    water[:, 5] = 1.0
    still = np.zeros((2 * len(hull), 3), f32)
    wet_counts = set()
    for _ in range(8):
        got = ctx.body_step(hull, got, props, step, 64)
        for _ in range(64):
            rec, _ = restate_dynamics(hull, want[:, :10], want[:, 10:16], oh.DRAG_LINEAR, water, still)
            want = np.concatenate([restate_step(rec, want, props, step), rec], axis=1)
            wet_counts.add(float(rec[0, 15]))
        np.testing.assert_array_equal(got, want)
    assert (got[:, 31] == want[:, 31]).all() and (got[:, 16] == want[:, 16]).all()
    assert (np.sign(got[:, 11]) == np.sign(want[:, 11])).all()
    print(f"after 512 substeps: y = {got[:, 1]}, v.y = {got[:, 11]}, wet = {got[:, 31]}, V = {got[:, 16]}")
    assert {0.0, 4.0} <= wet_counts  # the box started dry and went in
    assert 0.2 < got[0, 16] < 0.8 and abs(got[0, 1]) < 0.5  # about half submerged, near the surface
    np.testing.assert_array_equal(got[0, 3:7], f32(IDENTITY))  # the upright box gets no torque on flat water
    ctx.close()


def test_forms_and_ordering():
    """The async form equals the blocking one; a request made after step t1, with two more steps queued behind it,
    holds the answer of t1 (a second context gives it) and reads nothing of the caller's after the call; the launch is
    kind 2 and named."""
    n, cas = 128, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, V, times=()), make_ctx(n, cas, V, times=())
    rng = np.random.default_rng(4)
    hull, bodies, motion = oh.OceanContext.box_hull(5, 3, ny=2), random_bodies(rng, 300, 0.5), random_motion(rng, 300, 1.0)
    state, props, step = state_of(bodies, motion), random_props(rng, 300, hull), STEP.copy()
    h, s, p, sp = hull.copy(), state.copy(), props.copy(), step.copy()
    ctx.set_readback_timing(True)
    ctx.step(times[0])
    rb = ctx.body_step_async(h, s, p, sp, 4, law=oh.DRAG_QUADRATIC)
    h[:], s[:], p[:], sp[:] = 1.0e9, -1.0e9, 1.0e9, 7.0
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got, ms = rb.data.copy(), rb.copy_ms()
    rb.release()
    assert got.shape == (300, 32) and 0.0 < ms < 1000.0
    ref.step(times[0])
    np.testing.assert_array_equal(got, ref.body_step(hull, state, props, step, 4, law=oh.DRAG_QUADRATIC))
    later = ctx.body_step(hull, state, props, step, 4, law=oh.DRAG_QUADRATIC)  # the blocking form now: frame t3
    assert not np.array_equal(got[:, 16], later[:, 16]) and not np.array_equal(got[:, 1], later[:, 1])
    ctx.set_readback_timing(False)
    slot = oh.PinnedBuffer(300 * 128)
    for kw in (dict(), dict(iterations=0), dict(mode=oh.QUERY_REFERENCE, iterations=0)):
        rb = ctx.body_step_async(hull, state, props, step, 2, buf=slot, **kw)
        np.testing.assert_array_equal(rb.data, ctx.body_step(hull, state, props, step, 2, **kw))
        rb.release()
    slot.release()
    # counted as kind 2 and named
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)  # (reading resets the counters)
    ctx.body_step(hull, state, props, step, 8)
    ms, launches = ctx.kernel_stats(2)
    assert launches == 1 and ms > 0.0  # eight substeps, one launch
    ctx.set_kernel_timing(False)
    assert "k_body_step<32>" in ctx.kernel_name(2)  # 30 probes: 32 lanes per body
    ctx.close()
    ref.close()


def test_step_reads_a_later_tile():
    """On a context of three tiles, tile 2's result equals that of a single-tile context holding tile 2's noise, and
    differs from tile 0's."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V, tiles=3)
    one = make_ctx(n, cas, V, noise=O.generate_noise(n, 20251121 + 2))
    size, vmax = max_height(one.read_all(oh.TEX_DISP)), max_speed(one.read_all(oh.TEX_VELOCITY))
    rng = np.random.default_rng(23)
    hull, bodies, motion = random_hull(rng, 37, size), random_bodies(rng, M, size), random_motion(rng, M, vmax)
    state, props = state_of(bodies, motion), random_props(rng, M, hull)
    for kw in MODES:
        got = ctx.body_step(hull, state, props, STEP, 3, law=oh.DRAG_QUADRATIC, tile=2, **kw)
        np.testing.assert_array_equal(got, one.body_step(hull, state, props, STEP, 3, law=oh.DRAG_QUADRATIC, **kw))
        assert np.isfinite(got).all()
        assert not np.array_equal(got[:, 16], ctx.body_step(hull, state, props, STEP, 3, law=oh.DRAG_QUADRATIC, **kw)[:, 16])
    rb = ctx.body_step_async(hull, state, props, STEP, 3, law=oh.DRAG_QUADRATIC, tile=2)
    np.testing.assert_array_equal(rb.data, one.body_step(hull, state, props, STEP, 3, law=oh.DRAG_QUADRATIC))
    rb.release()
    ctx.close()
    one.close()


def test_step_refusals_on_a_live_context():
    """Without OCEAN_F_VELOCITY: E_UNSUPPORTED, behind the argument checks.  Before ocean_init_spectrum: E_STATE.  A
    misaligned device pointer, a tile out of range, the limits: E_INVALID_ARG.  None reaches a kernel.  count = 0 is a
    no-op in the blocking and device forms and refused by the async form."""
    import torch
    cas = O.SCENE_CASCADES[:2]
    hull, props = oh.OceanContext.box_hull(2, 2), np.ones((8, 4), f32)
    bodies = np.zeros((8, 10), f32)
    bodies[:, 3:7], bodies[:, 7:10] = IDENTITY, 1.0
    state = oh.OceanContext.body_state(bodies)
    plain = make_ctx(64, cas, 0, times=(1.0,))
    for call in (plain.body_step, plain.body_step_async):
        with pytest.raises(oh.OceanError) as e:
            call(hull, state, props, STEP)
        assert e.value.code == oh.E_UNSUPPORTED
    with pytest.raises(oh.OceanError) as e:  # the argument checks come first
        plain.body_step(hull, state, props, STEP, 0)
    assert e.value.code == oh.E_INVALID_ARG
    plain.close()
    ctx = oh.OceanContext(64, 2, 1, V)
    for call in (ctx.body_step, ctx.body_step_async):
        with pytest.raises(oh.OceanError) as e:
            call(hull, state, props, STEP)
        assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), cas)
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)
    nan_step = STEP.copy()
    nan_step[6] = np.nan
    bad = [dict(tile=1), dict(tile=-1), dict(mode=2), dict(iterations=17), dict(mode=oh.QUERY_REFERENCE, iterations=1),
           dict(law=2), dict(substeps=0), dict(substeps=oh.BODY_MAX_SUBSTEPS + 1), dict(step=nan_step)]
    for call in (ctx.body_step, ctx.body_step_async):
        for kw in bad:
            kw = dict(kw)
            with pytest.raises(oh.OceanError) as e:
                call(hull, state, props, kw.pop("step", STEP), **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
        many = oh.BODY_MAX_BODIES + 1
        for h, m, s in ((np.zeros((0, 5), f32), 8, 1),                          # probes < 1
                        (hull[:1], many, 1),                                    # count > the limit (staged forms)
                        (np.zeros((513, 5), f32), 8192, 1),                     # count * probes > 2^22
                        (np.zeros((512, 5), f32), 8192, 8)):                    # count * probes * substeps > 2^24
            with pytest.raises(oh.OceanError) as e:
                call(h, np.zeros((m, 32), f32), np.zeros((m, 4), f32), STEP, s)
            assert e.value.code == oh.E_INVALID_ARG, (h.shape, m, s)
    assert ctx.body_step(hull, np.zeros((0, 32), f32), np.zeros((0, 4), f32), STEP).shape == (0, 32)
    with pytest.raises(oh.OceanError) as e:
        ctx.body_step_async(hull, np.zeros((0, 32), f32), np.zeros((0, 4), f32), STEP)
    assert e.value.code == oh.E_INVALID_ARG
    # *req is NULL after a failure on a live context too
    out = np.zeros((8, 32), f32)
    req = ctypes.c_void_p(0x1234)
    assert ctx.lib.ocean_body_step_async(ctx._h, 0, oh.QUERY_SURFACE, 4, 0, 65, STEP.ctypes.data, hull.ctypes.data, 4,
                                         props.ctypes.data, state.ctypes.data, 8, out.ctypes.data,
                                         ctypes.byref(req)) == oh.E_INVALID_ARG
    assert req.value is None and not out.any()
    dev = torch.device("cuda", ctx.device)
    d_h = torch.zeros(4 * 5 + 1, dtype=torch.float32, device=dev)
    d_p = torch.zeros(8 * 4 + 1, dtype=torch.float32, device=dev)
    d_s = torch.zeros(8 * 32 + 4, dtype=torch.float32, device=dev)
    d_o = torch.zeros(8 * 32 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ph, pp, ps, po = d_h.data_ptr(), d_p.data_ptr(), d_s.data_ptr(), d_o.data_ptr()
    ctx.body_step_device(ph, 4, pp, ps, 0, po, STEP)
    # misaligned pointers are refused, not faulted on (in place too: out is then 4 B off a float4); count >
    # OCEAN_BODY_MAX_BODIES is not a limit of this form, the sample counts (in 64 bits) are
    for a in ((ph + 2, pp, ps, po), (ph, pp + 2, ps, po), (ph, pp, ps + 2, po), (ph, pp, ps, po + 4), (ph, pp, ps + 4, ps + 4)):
        with pytest.raises(oh.OceanError) as e:
            ctx.body_step_device(a[0], 4, a[1], a[2], 8, a[3], STEP)
        assert e.value.code == oh.E_INVALID_ARG, a
    for probes, count, s in ((1, oh.BODY_MAX_SAMPLES + 1, 1), (4096, 1 << 20, 64), (1, oh.BODY_MAX_SAMPLES, 8)):
        with pytest.raises(oh.OceanError) as e:
            ctx.body_step_device(ph, probes, pp, ps, count, po, STEP, s)
        assert e.value.code == oh.E_INVALID_ARG, (probes, count, s)
    ctx.synchronize()
    assert ctx.kernel_stats(2)[1] == 0  # none of the above reached a kernel
    ctx.set_kernel_timing(False)
    # the limits themselves are served by the staged forms (1232 KiB of inputs, 1 MiB of records): body b equals body
    # b alone
    rng = np.random.default_rng(2)
    big_hull = random_hull(rng, 512, 2.0)
    big = state_of(random_bodies(rng, oh.BODY_MAX_BODIES, 1.0), random_motion(rng, oh.BODY_MAX_BODIES, 1.0))
    big_props = random_props(rng, oh.BODY_MAX_BODIES, big_hull)
    rb = ctx.body_step_async(big_hull, big, big_props, STEP, 4)
    got = rb.data.copy()
    rb.release()
    assert got.shape == (oh.BODY_MAX_BODIES, 32) and np.isfinite(got).all()
    pick = [0, 1, 4097, 8191]
    np.testing.assert_array_equal(got[pick], ctx.body_step(big_hull, big[pick], big_props[pick], STEP, 4))
    ctx.close()
