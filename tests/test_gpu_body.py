"""GPU tests of the buoyant bodies (ocean_body_buoyancy / _device / _async, csrc/body.hip).  The entry is
restated here in numpy fp32 -- the transform and the per-probe terms as include/ocean/ocean.h orders them, the
surface lookup by restate_surface / restate_reference of tests/test_gpu_query.py over the context's own
read-back textures, the sum by tree_sum of tests/test_body_abi.py -- and the comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_body_abi import tree_sum
from test_gpu_query import Textures, make_ctx, restate_reference, restate_surface

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)
IDENTITY = (0.0, 0.0, 0.0, 1.0)


def cross(u, a):
    """(u x a) as ocean.h writes it: each component p * q - r * s, in that order."""
    return (u[1] * a[2] - u[2] * a[1], u[2] * a[0] - u[0] * a[2], u[0] * a[1] - u[1] * a[0])


def body_geometry(hull, bodies, dtype=f32):
    """d (the probes' offsets from the body origin, rotated and scaled), w (their world positions), h', v' as
    [M][P] arrays, in ocean.h's operation order (dtype float64: the same formulas, for the tolerance tests)."""
    h = np.asarray(hull, dtype)[None, :, :]
    b = np.asarray(bodies, dtype)[:, None, :]
    two = dtype(2.0)
    s = (b[..., 7], b[..., 8], b[..., 9])
    u, qw = (b[..., 3], b[..., 4], b[..., 5]), b[..., 6]
    a = (s[0] * h[..., 0], s[1] * h[..., 1], s[2] * h[..., 2])
    t = tuple(two * c for c in cross(u, a))
    ut = cross(u, t)
    d = tuple((a[i] + qw * t[i]) + ut[i] for i in range(3))
    w = tuple(b[..., i] + d[i] for i in range(3))
    hs = h[..., 3] * s[1]
    vs = ((h[..., 4] * s[0]) * s[1]) * s[2]
    return d, w, hs, vs


def restate_body(hull, bodies, lookup):
    """ocean_body_buoyancy: `lookup` maps q float32[M * P][2] to the [M * P][8] records the mode defines (height,
    -, -, r, n).  Returns (out float32[M][8], f float32[M][P])."""
    m, p = len(bodies), len(hull)
    d, w, hs, vs = body_geometry(hull, bodies)
    q = np.stack([w[0].ravel(), w[2].ravel()], axis=1)
    rec = lookup(q).reshape(m, p, 8)
    eta, r, n = rec[..., 0], rec[..., 3], rec[..., 4:7]
    half, zero, one = f32(0.5), f32(0.0), f32(1.0)
    bottom = w[1] - half * hs
    f = np.minimum(np.maximum((eta - bottom) / hs, zero), one)
    g = vs * f
    ey = (d[1] - half * hs) + half * (f * hs)
    terms = [g, g * d[0], g * ey, g * d[2], g * n[..., 0], g * n[..., 1], g * n[..., 2]]
    out = np.empty((m, 8), f32)
    for k, term in enumerate(terms):
        out[:, k] = tree_sum(term)
    out[:, 7] = r.max(axis=1)
    return out, f


def surface_lookup(tex, k):
    return lambda q: restate_surface(tex, q, (k,))[k]


def reference_lookup(disp0):
    def lookup(q):
        rec = restate_reference(disp0, q)
        rec[:, 1:] = f32([0, 0, 0, 0, 1, 0, 0])  # eta alone, n = (0, 1, 0), r = 0
        return rec
    return lookup


def random_quaternions(rng, m):
    q = rng.standard_normal((m, 4))
    return (q / np.linalg.norm(q, axis=1, keepdims=True)).astype(f32)


def random_bodies(rng, m, cy_scale, span=2000.0):
    """Random unit quaternions, scales in [0.5, 3], positions within +-span, cy within +-cy_scale."""
    b = np.empty((m, 10), f32)
    b[:, 0] = rng.uniform(-span, span, m)
    b[:, 1] = rng.uniform(-cy_scale, cy_scale, m)
    b[:, 2] = rng.uniform(-span, span, m)
    b[:, 3:7] = random_quaternions(rng, m)
    b[:, 7:10] = rng.uniform(0.5, 3.0, (m, 3))
    return b


def random_hull(rng, p, size):
    """P probes scattered over a box of side `size`, cells of height (0.5 .. 1.5) size and volume 0.1 .. 1."""
    h = np.empty((p, 5), f32)
    h[:, :3] = rng.uniform(-0.5, 0.5, (p, 3)) * size
    h[:, 3] = rng.uniform(0.5, 1.5, p) * size
    h[:, 4] = rng.uniform(0.1, 1.0, p)
    return h


def max_height(disp):
    """An upper bound of the summed height's magnitude: sum over the cascades of max |Dy|."""
    return float(sum(np.abs(disp[c][..., 1]).max() for c in range(disp.shape[0])))


# every W of the dispatch; 2, 12, 20 (W = 2, 16, 32) stand last so the random streams of the cases before them stay
PROBES = (1, 3, 8, 37, 64, 65, 130, 2, 12, 20)


@pytest.mark.parametrize("n,ncasc,flags", [(64, 1, 0), (64, 4, 0), (128, 2, oh.F_MIPS),
                                           (256, 3, oh.F_DISPLACEMENT_ONLY)])
def test_body_matches_restatement(n, ncasc, flags):
    """Bit-exact against the restatement: P in {1, 3, 8, 37, 64, 65, 130} (W = 1, 4, 8, 64 with one, two and three
    chunks; partial segments, partial waves, a partial last workgroup) and {2, 12, 20} (W = 2, 16, 32: with them
    every instantiation is launched), M = 37, K in {0, 4}, and reference mode.
    The poses put the hulls across the surface: over all probes of a context at least a quarter are partly
    submerged, 5 % dry and 5 % full, so the clamp cannot hide a wrong height."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = Textures(ctx, cas)
    size = max_height(tex.disp)
    assert size > 0.0
    rng = np.random.default_rng(1000 * n + ncasc)
    fractions = {0: [], 4: []}
    for p in PROBES:
        hull, bodies = random_hull(rng, p, size), random_bodies(rng, 37, size)
        for k in (0, 4):
            want, f = restate_body(hull, bodies, surface_lookup(tex, k))
            got = ctx.body_buoyancy(hull, bodies, iterations=k)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(got, want, err_msg=f"P = {p}, K = {k}")
            fractions[k].append(f.ravel())
        want, _ = restate_body(hull, bodies, reference_lookup(tex.disp[0]))
        got = ctx.body_buoyancy(hull, bodies, iterations=0, mode=oh.QUERY_REFERENCE)
        np.testing.assert_array_equal(got, want, err_msg=f"P = {p}, reference mode")
        if flags & oh.F_DISPLACEMENT_ONLY:  # no DERIV: n = (0, 1, 0), so the normal sums are (0, volume, 0)
            got = ctx.body_buoyancy(hull, bodies)
            np.testing.assert_array_equal(got[:, [4, 6]], np.zeros((37, 2), f32))
            np.testing.assert_array_equal(got[:, 5], got[:, 0])
    for k, fs in fractions.items():
        f = np.concatenate(fs)
        partial, dry, full = ((f > 0) & (f < 1)).mean(), (f == 0).mean(), (f == 1).mean()
        print(f"K = {k}: {len(f)} probes, partly submerged {partial:.3f}, dry {dry:.3f}, full {full:.3f}")
        assert partial >= 0.25 and dry >= 0.05 and full >= 0.05
    # the default arguments: surface mode, 4 steps
    np.testing.assert_array_equal(ctx.body_buoyancy(hull, bodies), ctx.body_buoyancy(hull, bodies, 4, oh.QUERY_SURFACE, 0))
    ctx.close()


def test_one_probe_is_the_query():
    """P = 1, the hull (0, 0, 0, h, v), the identity pose and scale 1: the probe sits at the body origin, so the
    record follows from ocean_query_surface at (cx, cz) by four fp32 operations.  M = 300: more than the 256
    one-lane bodies of a workgroup."""
    n, cas, m = 64, O.SCENE_CASCADES[:2], 300
    ctx = make_ctx(n, cas)
    size = max_height(ctx.read_all(oh.TEX_DISP))
    rng = np.random.default_rng(5)
    h, v = f32(1.25 * size), f32(0.75)
    hull = f32([[0, 0, 0, h, v]])
    bodies = random_bodies(rng, m, size)
    bodies[:, 3:7], bodies[:, 7:10] = IDENTITY, 1.0
    cy = bodies[:, 1]
    q = np.ascontiguousarray(bodies[:, [0, 2]])

    def expect(eta):
        f = np.minimum(np.maximum((eta - (cy - f32(0.5) * h)) / h, f32(0)), f32(1))
        return f, v * f

    for k in (0, 4):
        rec = ctx.query_surface(q, iterations=k)
        got = ctx.body_buoyancy(hull, bodies, iterations=k)
        f, g = expect(rec[:, 0])
        assert ((f > 0) & (f < 1)).mean() > 0.25
        np.testing.assert_array_equal(got[:, 0], g)
        np.testing.assert_array_equal(got[:, 7], rec[:, 3])
        np.testing.assert_array_equal(got[:, 4:7], g[:, None] * rec[:, 4:7])
        np.testing.assert_array_equal(got[:, [1, 3]], np.zeros((m, 2), f32))  # the probe is at the origin: d = 0
        np.testing.assert_array_equal(got[:, 2], g * ((f32(0) - f32(0.5) * h) + f32(0.5) * (f * h)))
    # reference mode: GetWaterHeight's texel, n = (0, 1, 0), r = 0; positions across [-N/2, N/2] and beyond it
    bodies[:, [0, 2]] = rng.uniform(-n / 2 - 3, n / 2 + 3, (m, 2))
    q = np.ascontiguousarray(bodies[:, [0, 2]])
    with pytest.raises(oh.OceanError) as e:
        ctx.body_buoyancy(hull, bodies, iterations=1, mode=oh.QUERY_REFERENCE)
    assert e.value.code == oh.E_INVALID_ARG
    got = ctx.body_buoyancy(hull, bodies, iterations=0, mode=oh.QUERY_REFERENCE)
    eta = restate_reference(ctx.read(oh.TEX_DISP, 0, 0), q)[:, 0]
    np.testing.assert_array_equal(eta, ctx.query_surface(q, mode=oh.QUERY_REFERENCE, iterations=0)[:, 0])
    f, g = expect(eta)
    assert ((f > 0) & (f < 1)).mean() > 0.25
    np.testing.assert_array_equal(got[:, 0], g)
    np.testing.assert_array_equal(got[:, 4:7], np.stack([g * f32(0), g, g * f32(0)], axis=1))
    np.testing.assert_array_equal(got[:, 7], np.zeros(m, f32))
    ctx.close()


def test_known_answers_high_and_deep():
    """Bodies far above the water displace nothing; bodies far below it displace their whole hull: out[0] is the
    tree sum of v', whatever the rotation, and out[1..3] is the rotated first moment R (sum v' a) -- for the
    symmetric box zero -- within 8 eps sum v' |a| (|a| Euclidean).  out[7], the residual, does not depend on the
    depth: the probes of the high and the deep bodies stand over the same (x, z)."""
    n, cas, m = 64, O.SCENE_CASCADES[:2], 37
    ctx = make_ctx(n, cas)
    rng = np.random.default_rng(9)
    box = oh.OceanContext.box_hull(8, 8)
    lopsided = box.copy()
    lopsided[:, 0] += f32(0.375)  # the same cells about another origin: the first moment is not zero
    lopsided[:, 4] *= rng.uniform(0.5, 1.5, len(box)).astype(f32)
    for hull in (box, lopsided):
        bodies = random_bodies(rng, m, 0.0)
        bodies[:, 7:10] = bodies[0, 7:10]  # one scale, so that one volume, under 37 rotations
        bodies[:, 1] = 1000.0
        high = ctx.body_buoyancy(hull, bodies)
        np.testing.assert_array_equal(high[:, :7], np.zeros((m, 7), f32))
        bodies[:, 1] = -1000.0
        deep = ctx.body_buoyancy(hull, bodies)
        np.testing.assert_array_equal(deep[:, 7], high[:, 7])
        assert high[:, 7].max() > 0.0
        _, _, _, vs = body_geometry(hull, bodies)
        np.testing.assert_array_equal(deep[:, 0], tree_sum(vs))
        assert len(set(deep[:, 0].tolist())) == 1  # bit-identical for every rotation
        d64, _, _, vs64 = body_geometry(hull, bodies, np.float64)  # linear in a: sum v' d = R (sum v' a)
        sx, sy, sz = bodies[0, 7:10].astype(np.float64)
        norm_a = np.sqrt((sx * hull[:, 0]) ** 2 + (sy * hull[:, 1]) ** 2 + (sz * hull[:, 2]) ** 2)
        bound = 8 * EPS32 * float((vs64[0] * norm_a).sum())
        want = np.stack([(vs64 * d64[i]).sum(axis=1) for i in range(3)], axis=1)
        err = np.abs(deep[:, 1:4].astype(np.float64) - want).max()
        print(f"first moment: max error {err:.3e}, bound {bound:.3e}, max |moment| {np.abs(want).max():.3e}")
        assert err <= bound
        if hull is box:
            assert np.abs(deep[:, 1:4]).max() <= bound
        else:
            assert np.abs(want).max() > 1000 * bound
    ctx.close()


def test_rolled_box_gets_a_restoring_torque():
    """A box of 8 x 8 probes centred on the waterline of a calm sea (the scene's noise scaled by 1e-3: waves of
    millimetres), rolled by +-0.2 rad about z: half of it is under water, the side that went down displaces
    more, and the torque about z opposes the roll."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, noise=O.generate_noise(n, 20251121) * f32(1e-3))
    size = (4.0, 2.0, 4.0)  # metres; the height is size[1]
    disp = ctx.read_all(oh.TEX_DISP)
    dmax = float(sum(np.abs(disp[c][..., :3]).max() for c in range(len(cas))))
    print(f"calm sea: sum_c max |D| = {dmax:.3e} m")
    assert 0.0 < dmax < 0.01 * size[1]
    hull = oh.OceanContext.box_hull(8, 8)
    bodies = np.zeros((3, 10), f32)
    bodies[:, 0], bodies[:, 2] = 12.5, -40.0
    bodies[:, 7:10] = size
    for b, roll in enumerate((0.2, -0.2, 0.0)):
        bodies[b, 3:7] = (0.0, 0.0, np.sin(roll / 2), np.cos(roll / 2))
    out = ctx.body_buoyancy(hull, bodies)
    force, point, torque = oh.OceanContext.buoyancy_wrench(out, 1000.0, 9.81)
    volume = size[0] * size[1] * size[2]
    print(f"volumes {out[:, 0]}, torque z {torque[:, 2]}, points {point.tolist()}")
    assert (np.abs(out[:, 0] / (0.5 * volume) - 1.0) < 0.02).all()
    assert torque[0, 2] < 0.0 < torque[1, 2]  # opposes the roll, and flips with it
    # the column model's own answer for this box: -rho g V_box sx^2 (1 - 1 / 64) sin(2 roll) / 48, to the waves
    want = -1000.0 * 9.81 * volume * size[0] ** 2 * (1 - 1 / 64) * np.sin(0.4) / 48
    assert abs(torque[0, 2] / want - 1.0) < 0.02 and abs(torque[1, 2] / -want - 1.0) < 0.02
    assert abs(torque[2, 2]) < 0.02 * abs(want)  # level: no torque beyond the waves'
    assert (point[:, 1] < 0.0).all()  # the centre of buoyancy lies below the waterline
    normal = out[:, 4:7] / np.linalg.norm(out[:, 4:7], axis=1, keepdims=True)
    assert (normal[:, 1] > 0.999).all()
    ctx.close()


def test_body_errors_limits_and_device_form():
    import torch
    hull, bodies = oh.OceanContext.box_hull(2, 2), np.zeros((8, 10), f32)
    bodies[:, 3:7], bodies[:, 7:10] = IDENTITY, 1.0
    ctx = oh.OceanContext(64, 2, 1)
    for call in (ctx.body_buoyancy, ctx.body_buoyancy_async):
        with pytest.raises(oh.OceanError) as e:
            call(hull, bodies)
        assert e.value.code == oh.E_STATE  # before ocean_init_spectrum
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    bad = [dict(tile=1), dict(tile=-1), dict(mode=2), dict(mode=-1), dict(iterations=17), dict(iterations=-1),
           dict(mode=oh.QUERY_REFERENCE, iterations=1)]
    for call in (ctx.body_buoyancy, ctx.body_buoyancy_async):
        for kw in bad:
            with pytest.raises(oh.OceanError) as e:
                call(hull, bodies, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
        for h, b in ((np.zeros((0, 5), f32), bodies),                              # probes < 1
                     (np.zeros((oh.BODY_MAX_PROBES + 1, 5), f32), bodies),         # probes > the limit
                     (hull[:1], np.zeros((oh.BODY_MAX_BODIES + 1, 10), f32)),      # count > the limit
                     (np.zeros((513, 5), f32), np.zeros((8192, 10), f32))):        # count * probes > 2^22
            with pytest.raises(oh.OceanError) as e:
                call(h, b)
            assert e.value.code == oh.E_INVALID_ARG, (h.shape, b.shape)
    # nulls and a negative count, through the C entries themselves; *req is reset
    lib, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    out = np.zeros((8, 8), f32)
    hp, bp, op = hull.ctypes.data, bodies.ctypes.data, out.ctypes.data
    for args in ((None, 4, bp, 8, op), (hp, 4, None, 8, op), (hp, 4, bp, 8, None), (hp, 4, bp, -1, op)):
        for name in ("ocean_body_buoyancy", "ocean_body_buoyancy_device"):
            assert getattr(lib, name)(h, 0, oh.QUERY_SURFACE, 4, *args) == oh.E_INVALID_ARG, (name, args)
        req = vp(0x1234)
        assert lib.ocean_body_buoyancy_async(h, 0, oh.QUERY_SURFACE, 4, *args, ctypes.byref(req)) == oh.E_INVALID_ARG
        assert req.value is None
    assert lib.ocean_body_buoyancy_async(h, 0, oh.QUERY_SURFACE, 4, hp, 4, bp, 8, op, None) == oh.E_INVALID_ARG
    assert not out.any()
    # count = 0: a no-op in the blocking form, but no request to hand back
    assert ctx.body_buoyancy(hull, np.zeros((0, 10), f32)).shape == (0, 8)
    with pytest.raises(oh.OceanError) as e:
        ctx.body_buoyancy_async(hull, np.zeros((0, 10), f32))
    assert e.value.code == oh.E_INVALID_ARG
    # the limits themselves are served: 8192 bodies of 512 probes are 2^22 samples; body b equals body b alone
    rng = np.random.default_rng(2)
    big_hull, big = random_hull(rng, 512, 2.0), random_bodies(rng, oh.BODY_MAX_BODIES, 1.0)
    got = ctx.body_buoyancy(big_hull, big)
    assert got.shape == (oh.BODY_MAX_BODIES, 8) and np.isfinite(got).all()
    pick = [0, 1, 4097, 8191]
    np.testing.assert_array_equal(got[pick], ctx.body_buoyancy(big_hull, big[pick]))
    # the device form: async on the ctx stream; equal to the blocking form; misaligned pointers are refused
    dev = torch.device("cuda", ctx.device)
    bodies = random_bodies(rng, 8, 1.0, span=100.0)
    dh = torch.zeros(4 * 5 + 1, dtype=torch.float32, device=dev)
    dh[:20] = torch.from_numpy(hull.ravel()).to(dev)
    db = torch.zeros(8 * 10 + 1, dtype=torch.float32, device=dev)
    db[:80] = torch.from_numpy(bodies.ravel()).to(dev)
    o = torch.zeros(8 * 8 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.body_buoyancy_device(dh.data_ptr(), 4, db.data_ptr(), 8, o.data_ptr())
    ctx.body_buoyancy_device(dh.data_ptr(), 4, db.data_ptr(), 0, o.data_ptr())  # count = 0: a no-op
    misaligned = [(dh.data_ptr() + 2, db.data_ptr(), o.data_ptr()), (dh.data_ptr(), db.data_ptr() + 2, o.data_ptr()),
                  (dh.data_ptr(), db.data_ptr(), o.data_ptr() + 4)]
    for ph, pb, po in misaligned:
        with pytest.raises(oh.OceanError) as e:
            ctx.body_buoyancy_device(ph, 4, pb, 8, po)
        assert e.value.code == oh.E_INVALID_ARG
    # count * probes is checked in 64 bits, also where the body limit does not apply: 2^20 * 4096 = 2^32
    for probes, count in ((1, oh.BODY_MAX_SAMPLES + 1), (4096, 1 << 20), (4096, 1025)):
        with pytest.raises(oh.OceanError) as e:
            ctx.body_buoyancy_device(dh.data_ptr(), probes, db.data_ptr(), count, o.data_ptr())
        assert e.value.code == oh.E_INVALID_ARG, (probes, count)
    ctx.synchronize()
    np.testing.assert_array_equal(o[:64].cpu().numpy().reshape(8, 8), ctx.body_buoyancy(hull, bodies))
    assert not o[64:].cpu().numpy().any()
    ctx.close()


def test_body_async_snapshots_behind_later_steps():
    """ocean_body_buoyancy_async: the request made after step t1, with two more steps queued right behind it,
    holds the answer of t1 (a second context gives it); the caller's hull and bodies, overwritten right after
    the call, are not read again; with readback timing on, the request reports its copy time."""
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
    rng = np.random.default_rng(4)
    hull, bodies = oh.OceanContext.box_hull(5, 3, ny=2), random_bodies(rng, 300, 0.5)
    h, b = hull.copy(), bodies.copy()
    ctx.set_readback_timing(True)
    ctx.step(times[0])
    rb = ctx.body_buoyancy_async(h, b)
    h[:], b[:] = 1.0e9, -1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    ms = rb.copy_ms()
    rb.release()
    assert got.shape == (300, 8) and 0.0 < ms < 1000.0
    ref.step(times[0])
    np.testing.assert_array_equal(got, ref.body_buoyancy(hull, bodies))
    later = ctx.body_buoyancy(hull, bodies)  # the blocking form now: frame t3
    assert not np.array_equal(got[:, 0], later[:, 0])
    # the async form equals the blocking form bit for bit; reference mode and a caller-owned pinned slot
    ctx.set_readback_timing(False)
    slot = oh.PinnedBuffer(len(bodies) * 32)
    for kw in (dict(), dict(iterations=0), dict(mode=oh.QUERY_REFERENCE, iterations=0)):
        rb = ctx.body_buoyancy_async(hull, bodies, buf=slot, **kw)
        np.testing.assert_array_equal(rb.data, ctx.body_buoyancy(hull, bodies, **kw))
        with pytest.raises(oh.OceanError) as e:
            rb.copy_ms()
        assert e.value.code == oh.E_STATE  # made with readback timing off
        rb.release()
    slot.release()
    ctx.close()
    ref.close()


def test_body_launch_is_counted_and_named():
    ctx = make_ctx(64, O.SCENE_CASCADES[:2])
    hull, bodies = oh.OceanContext.box_hull(3, 3), random_bodies(np.random.default_rng(1), 10, 1.0)
    ctx.set_kernel_timing(True)
    ctx.kernel_stats(2)  # (reading resets the counters)
    ctx.body_buoyancy(hull, bodies)
    ms, launches = ctx.kernel_stats(2)
    assert launches == 1 and ms > 0.0
    ctx.set_kernel_timing(False)
    assert "k_body_buoyancy<16>" in ctx.kernel_name(2)  # 9 probes: 16 lanes per body
    ctx.close()
