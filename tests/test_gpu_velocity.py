"""GPU tests of the surface velocity (OCEAN_F_VELOCITY, csrc/velocity.hip): the VELOCITY texture against the
oracle's transform of velocity_planes (tests/test_velocity_abi.py) formed from the context's own H0 and WAVES,
the finite-difference condition on the context's own DISP where no CPU transform exists (N = 4096), the same
parity over several tiles, in shallow water, with the operator chunked inside the scratch and with the streamed
pack, the absence of side effects on the frame, and ocean_query_velocity / _device / _async bit for bit against a numpy
restatement on top of the surface query's (tests/test_gpu_query.py)."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_parity import _ctx_with_env
from test_gpu_parity import make_ctx as parity_ctx
from test_gpu_query import KS, Textures, make_ctx, restate_surface
from test_gpu_sample import _points
from test_velocity_abi import finite_difference_bound, velocity_texture

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
V = oh.F_VELOCITY


@pytest.mark.parametrize("n,ncasc,flags", [(16, 2, 0), (64, 2, 0), (128, 2, 0), (256, 2, 0), (1024, 1, 0),
                                           (128, 2, oh.F_UNFUSED), (128, 2, oh.F_DISPLACEMENT_ONLY),
                                           (128, 2, oh.F_MIPS)])
def test_velocity_texture_parity(n, ncasc, flags):
    """VEL read back against O.ifft2d(velocity_planes(H0, WAVES, t)) from the context's own H0 and WAVES, at
    t = 1.25 and t = 100: the project's parity tolerance, every channel and cascade."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags | V, times=())
    np.testing.assert_array_equal(ctx.read_all(oh.TEX_VELOCITY), 0)  # zero after create
    h0, w = ctx.read_all(oh.TEX_H0), ctx.read_all(oh.TEX_WAVES)
    for t in (1.25, 100.0):
        ctx.step(t)
        got = ctx.read_all(oh.TEX_VELOCITY)
        want = velocity_texture(h0, w, t)
        assert np.abs(want[..., :3]).max() > 0
        for c in range(ncasc):
            for ch in range(4):
                e = O.rel_err(got[c, ..., ch], want[c, ..., ch])
                print(f"N = {n}, flags {flags:#x}, t = {t}, cascade {c}, channel {ch}: rel err {e:.2e}")
                assert e <= 1e-5, (n, flags, t, c, ch, e)
    ptr, nbytes = ctx.device_ptr(oh.TEX_VELOCITY)
    assert ptr and nbytes == ncasc * n * n * 16
    ctx.close()


def check_velocity_parity(ctx, tile, t):
    """VEL of `tile` at the time t of the last step against velocity_texture of that tile's own H0 and WAVES:
    the parity tolerance, every channel and cascade."""
    got = ctx.read_all(oh.TEX_VELOCITY, tile)
    want = velocity_texture(ctx.read_all(oh.TEX_H0, tile), ctx.read_all(oh.TEX_WAVES, tile), t)
    assert np.abs(want[..., :3]).max() > 0
    for c in range(ctx.C):
        for ch in range(4):
            e = O.rel_err(got[c, ..., ch], want[c, ..., ch])
            print(f"N = {ctx.n}, tile {tile}, t = {t}, cascade {c}, channel {ch}: rel err {e:.2e}")
            assert e <= 1e-5, (ctx.n, tile, t, c, ch, e)


@pytest.mark.parametrize("n,ncasc,tiles", [(64, 2, 3), (128, 4, 2), (512, 2, 2)])
def test_velocity_texture_parity_over_tiles(n, ncasc, tiles):
    """U = T * C units with their own noise per tile: k_evolve_velocity and k_pack_velocity over every unit, the
    [2][U] plane-major scratch and the operator over its 2 U unit-planes.  Every tile's VEL against that
    tile's own spectrum at the parity tolerance, at t = 1.25 and t = 100; the tiles' VEL differ."""
    ctx = make_ctx(n, O.SCENE_CASCADES[:ncasc], V, times=(), tiles=tiles)
    for t in (1.25, 100.0):
        ctx.step(t)
        for tile in range(tiles):
            check_velocity_parity(ctx, tile, t)
    vel = [ctx.read_all(oh.TEX_VELOCITY, tile) for tile in range(tiles)]
    for a in range(tiles):
        for b in range(a + 1, tiles):
            for c in range(ncasc):
                assert not np.array_equal(vel[a][c], vel[b][c]), (a, b, c)
    ptr, nbytes = ctx.device_ptr(oh.TEX_VELOCITY)
    assert ptr and nbytes == tiles * ncasc * n * n * 16
    ctx.close()


def test_velocity_texture_parity_shallow():
    """Depth 4 (the shallow scene of test_gpu_parity.test_shallow_frames_vs_oracle): the TMA correction and the
    finite-depth dw/dk reach the velocity path through H0.  omega itself stays the deep-water sqrt(g k) at every
    depth, as in the reference (InitialSpectrum.compute:33-35): WAVES is the deep scene's, H0 is not."""
    n, cas = 128, O.SCENE_CASCADES[:2]
    deep, _ = parity_ctx(n, cas, flags=V)
    ctx, _ = parity_ctx(n, cas, params=O.scene_params(shallow=True), flags=V)
    np.testing.assert_array_equal(ctx.read_all(oh.TEX_WAVES), deep.read_all(oh.TEX_WAVES))
    assert not np.array_equal(ctx.read_all(oh.TEX_H0), deep.read_all(oh.TEX_H0))
    deep.close()
    for t in (1.25, 100.0):
        ctx.step(t)
        check_velocity_parity(ctx, 0, t)
    ctx.close()


def test_velocity_operator_chunks():
    """OCEAN_OP_CHUNK_MIB (read per context in ocean_create) = 6 at N = 512 with U = 4: a unit-plane is 2 MiB,
    so the operator takes the 8 unit-planes of the [2][U] scratch as 3 + 3 + 2 -- one chunk straddles the
    v0 / v1 boundary, one is partial.  Per step that is evolve + 3 x (rows, columns) + pack = 8 launches of
    kind 2 against 4 in one chunk; VEL is bit-identical, and DISP, DERIV and TURB equal a plain context's."""
    n, cas, tiles = 512, O.SCENE_CASCADES[:2], 2
    res = []
    for env, flags in (({"OCEAN_OP_CHUNK_MIB": "6"}, V), ({"OCEAN_OP_CHUNK_MIB": "0"}, V), ({}, 0)):
        ctx, _ = _ctx_with_env(env, n, cas, tiles=tiles, flags=flags)
        ctx.set_kernel_timing(True)
        for t in (0.5, 1.0):
            ctx.step(t)
        launches = ctx.kernel_stats(2)[1]
        ctx.set_kernel_timing(False)
        texs = (oh.TEX_DISP, oh.TEX_DERIV, oh.TEX_TURB) + ((oh.TEX_VELOCITY,) if flags else ())
        res.append((launches, [[ctx.read_all(tex, tile) for tile in range(tiles)] for tex in texs]))
        ctx.close()
    (n_chunked, chunked), (n_whole, whole), (n_plain, plain) = res
    assert n_whole == n_plain + 2 * 4 and n_chunked == n_plain + 2 * 8
    assert np.abs(whole[3][1]).max() > 0
    np.testing.assert_array_equal(chunked[3], whole[3])
    for a, b, c in zip(chunked[:3], whole[:3], plain):
        np.testing.assert_array_equal(a, c)
        np.testing.assert_array_equal(b, c)


def test_velocity_streamed_pack():
    """OCEAN_VEL_NT=1 selects k_pack_velocity<true>, the pack with streamed stores: the same VEL bit for bit,
    over 2 tiles x 2 cascades at N = 128 after two steps."""
    n, cas, tiles = 128, O.SCENE_CASCADES[:2], 2
    res = []
    for env, kernel in (({"OCEAN_VEL_NT": "1"}, "k_pack_velocity<true>"), ({}, "k_pack_velocity<false>")):
        ctx, _ = _ctx_with_env(env, n, cas, tiles=tiles, flags=V)
        for t in (0.5, 1.0):
            ctx.step(t)
        assert kernel in ctx.kernel_name(2)  # the step's last launch
        res.append([ctx.read_all(oh.TEX_VELOCITY, tile) for tile in range(tiles)])
        ctx.close()
    assert np.abs(res[1][1]).max() > 0
    np.testing.assert_array_equal(res[0], res[1])


def test_velocity_4096_is_the_derivative_of_disp():
    """N = 4096 (the folded operator): no CPU transform of that size, so the finite-difference condition of
    tests/test_velocity_abi.py on the context's own DISP at t = 1 +- 1/256 against VEL at t = 1, x, y, z.
    The CPU oracle gives 3.5e-5 against the bound of 5.4e-4."""
    n, t, dt = 4096, 1.0, 1.0 / 256.0
    ctx = oh.OceanContext(n, 1, 1, V)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    ctx.generate_noise_device(1)
    ctx.init_spectrum()
    ctx.step(t - dt)
    lo = ctx.read(oh.TEX_DISP)[..., :3]
    ctx.step(t + dt)
    hi = ctx.read(oh.TEX_DISP)[..., :3]
    ctx.step(t)
    vel = ctx.read(oh.TEX_VELOCITY)
    omega_max = ctx.read(oh.TEX_WAVES)[..., 3].max()
    ctx.close()
    bound = finite_difference_bound(omega_max, t, dt)
    for ch, name in enumerate("xyz"):
        fd = (hi[..., ch].astype(np.float64) - lo[..., ch]) / (2.0 * dt)
        e = O.rel_err(vel[..., ch], fd)
        print(f"N = 4096, {name}: rel err {e:.3e}, bound {bound:.3e}")
        assert e <= bound, (name, e, bound)


@pytest.mark.parametrize("n,ncasc,flags", [(128, 2, 0), (512, 2, 0), (128, 2, oh.F_UNFUSED)])
def test_velocity_leaves_the_frame_alone(n, ncasc, flags):
    """A velocity context's DISP, DERIV and TURB after three steps equal a plain context's bit for bit, and
    its kind 0 and kind 1 launch counts are the plain context's: the velocity launches are kind 2."""
    cas = O.SCENE_CASCADES[:ncasc]
    res = []
    for fl in (flags, flags | V):
        ctx = make_ctx(n, cas, fl, times=())
        ctx.set_kernel_timing(True)
        for t in (0.25, 0.5, 0.75):
            ctx.step(t)
        counts = [ctx.kernel_stats(k)[1] for k in range(3)]
        ctx.set_kernel_timing(False)
        res.append((counts, [ctx.read_all(tex) for tex in (oh.TEX_DISP, oh.TEX_DERIV, oh.TEX_TURB)],
                    ctx.step_bytes()))
        ctx.close()
    (plain_counts, plain_tex, plain_bytes), (vel_counts, vel_tex, vel_bytes) = res
    assert vel_counts[:2] == plain_counts[:2] and plain_counts[0] > 0 and plain_counts[1] > 0
    assert vel_counts[2] == plain_counts[2] + 3 * 4  # evolve, rows, columns, pack per step
    assert vel_bytes == plain_bytes
    for a, b in zip(plain_tex, vel_tex):
        np.testing.assert_array_equal(a, b)


def restate_velocity(tex, vel, q, ks):
    """ocean_query_velocity for every K in `ks`: the surface query's iteration (restate_surface) and the
    cascade-summed bilinear taps of VEL at the point it ends on, in ocean.h's order: {K: [M][8]}."""
    surf = restate_surface(tex, q, ks)
    out = {}
    for k in ks:
        p = surf[k][:, 1:3]
        vs = np.zeros((len(p), 4), f32)
        for c, L in enumerate(tex.lengths):
            L = f32(L)
            vs = vs + O._tap(vel[c], p[:, 0] / L, p[:, 1] / L)
        out[k] = np.stack([vs[:, 0], vs[:, 1], vs[:, 2], surf[k][:, 3], surf[k][:, 0], p[:, 0], p[:, 1], vs[:, 3]], axis=1)
    return out


@pytest.mark.parametrize("n,ncasc", [(64, 1), (64, 4), (128, 2)])
def test_query_velocity_matches_restatement(n, ncasc):
    """Bit for bit against the restatement for K in {0, 1, 4, 16}; (64, 4) is the folding scene.  The record
    shares its residual, height and point with the surface query's; K = 0 samples at q itself."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, V)
    q = np.ascontiguousarray(_points(4096, n, n + ncasc)[:, :2])
    want = restate_velocity(Textures(ctx, cas), ctx.read_all(oh.TEX_VELOCITY), q, KS)
    got = {}
    for k in KS:
        got[k] = ctx.query_velocity(q, iterations=k)
        assert np.isfinite(got[k]).all()
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"K = {k}")
        np.testing.assert_array_equal(got[k][:, 3:7], ctx.query_surface(q, iterations=k)[:, [3, 0, 1, 2]])
    np.testing.assert_array_equal(got[0][:, 5:7], q)
    assert np.abs(got[4][:, :3]).max() > 0
    np.testing.assert_array_equal(ctx.query_velocity(q), got[4])  # the default: 4 steps
    ctx.close()


def test_query_velocity_before_the_first_step_is_zero():
    """VEL is zero after create and the query is valid: the four velocity components are +0."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, V, times=())
    q = np.ascontiguousarray(_points(512, n, 3)[:, :2])
    for k in (0, 4):
        got = ctx.query_velocity(q, iterations=k)
        vel = got[:, [0, 1, 2, 7]]
        assert not vel.any() and not np.signbit(vel).any()
        np.testing.assert_array_equal(got[:, 3:7], ctx.query_surface(q, iterations=k)[:, [3, 0, 1, 2]])
    ctx.close()


def test_query_velocity_forms_agree_and_async_snapshots():
    """The device and async forms equal the blocking one bit for bit; an async request issued between two
    steps sees the first step's VEL (a second context gives it), and its points are consumed by the call."""
    import torch
    n, cas = 128, O.SCENE_CASCADES[:2]
    ctx, ref = make_ctx(n, cas, V, times=()), make_ctx(n, cas, V, times=())
    q = np.ascontiguousarray(_points(1000, n, 5)[:, :2])
    buf = q.copy()
    ctx.step(0.25)
    rb = ctx.query_velocity_async(buf)
    buf[:] = 1.0e9
    ctx.step(0.5)
    rb.wait()
    got = rb.data
    rb.release()
    ref.step(0.25)
    np.testing.assert_array_equal(got, ref.query_velocity(q))
    later = ctx.query_velocity(q)  # the blocking query now: the second step
    assert not np.array_equal(got[:, :3], later[:, :3])
    slot = oh.PinnedBuffer(len(q) * 32)  # a caller-owned pinned slot, other iterations
    rb = ctx.query_velocity_async(q, iterations=1, buf=slot)
    np.testing.assert_array_equal(rb.data, ctx.query_velocity(q, iterations=1))
    rb.release()
    slot.release()
    dev = torch.device("cuda", ctx.device)
    d_q = torch.from_numpy(q).to(dev)
    d_out = torch.zeros(len(q) * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.query_velocity_device(d_q.data_ptr(), len(q), d_out.data_ptr())
    ctx.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().reshape(-1, 8), later)
    ctx.close()
    ref.close()


def test_velocity_errors():
    import torch
    pts = np.zeros((8, 2), f32)
    cas = O.SCENE_CASCADES[:2]
    # a context without the flag: no texture, no query
    n = 256
    plain = make_ctx(n, cas, 0, times=(1.0,))
    for call in (plain.query_velocity, plain.query_velocity_async):
        with pytest.raises(oh.OceanError) as e:
            call(pts)
        assert e.value.code == oh.E_UNSUPPORTED
    dev = torch.device("cuda", plain.device)
    d_p = torch.zeros(8 * 2 + 1, dtype=torch.float32, device=dev)
    d_o = torch.zeros(8 * 8 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    with pytest.raises(oh.OceanError) as e:
        plain.query_velocity_device(d_p.data_ptr(), 8, d_o.data_ptr())
    assert e.value.code == oh.E_UNSUPPORTED
    for call in (lambda: plain.read(oh.TEX_VELOCITY), lambda: plain.read_async(oh.TEX_VELOCITY),
                 lambda: plain.device_ptr(oh.TEX_VELOCITY),
                 lambda: plain.write(oh.TEX_VELOCITY, np.zeros((n, n, 4), f32))):
        with pytest.raises(oh.OceanError) as e:
            call()
        assert e.value.code == oh.E_INVALID_ARG
    plain.set_column_band(0, n // 2)  # a plain context still takes a band
    plain.close()
    # a velocity context before ocean_init_spectrum
    ctx = oh.OceanContext(n, 2, 1, V)
    for call in (ctx.query_velocity, ctx.query_velocity_async):
        with pytest.raises(oh.OceanError) as e:
            call(pts)
        assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), cas)
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    for kw in (dict(tile=1), dict(tile=-1), dict(iterations=17), dict(iterations=-1)):
        for call in (ctx.query_velocity, ctx.query_velocity_async):
            with pytest.raises(oh.OceanError) as e:
                call(pts, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
    many = np.zeros((oh.QUERY_MAX_POINTS + 1, 2), f32)
    for call in (ctx.query_velocity, ctx.query_velocity_async):
        with pytest.raises(oh.OceanError) as e:
            call(many)
        assert e.value.code == oh.E_INVALID_ARG
    assert ctx.query_velocity(many[:-1]).shape == (oh.QUERY_MAX_POINTS, 8)  # the maximum itself is served
    assert ctx.query_velocity(np.zeros((0, 2), f32)).shape == (0, 8)  # count 0: a no-op
    with pytest.raises(oh.OceanError) as e:
        ctx.query_velocity_async(np.zeros((0, 2), f32))  # ... but no request to hand back
    assert e.value.code == oh.E_INVALID_ARG
    # the device form refuses misaligned pointers instead of faulting on them; count 0 is a no-op
    lib, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    assert lib.ocean_query_velocity_device(h, 0, 4, vp(d_p.data_ptr()), 8, vp(d_o.data_ptr() + 4)) == oh.E_INVALID_ARG
    assert lib.ocean_query_velocity_device(h, 0, 4, vp(d_p.data_ptr() + 2), 8, vp(d_o.data_ptr())) == oh.E_INVALID_ARG
    assert lib.ocean_query_velocity_device(h, 0, 4, vp(d_p.data_ptr()), 0, vp(d_o.data_ptr())) == oh.OK
    assert lib.ocean_query_velocity_device(h, 0, 4, vp(d_p.data_ptr()), 8, vp(d_o.data_ptr())) == oh.OK
    ctx.synchronize()
    # VELOCITY is written like NORMAL, a derived output: the upload lands and the next step replaces it
    ones = np.ones((n, n, 4), f32)
    ctx.write(oh.TEX_VELOCITY, ones, cascade=1)
    np.testing.assert_array_equal(ctx.read(oh.TEX_VELOCITY, cascade=1), ones)
    # no band and no parity on a velocity context; the whole band and "off" are accepted
    for call in (lambda: ctx.set_column_band(0, n // 2), lambda: ctx.set_column_band(n // 2, n // 2),
                 lambda: ctx.set_column_parity(0), lambda: ctx.set_column_parity(1)):
        with pytest.raises(oh.OceanError) as e:
            call()
        assert e.value.code == oh.E_UNSUPPORTED
    ctx.set_column_band(0, n)
    ctx.set_column_parity(-1)
    ctx.step(1.0)
    assert not np.array_equal(ctx.read(oh.TEX_VELOCITY, cascade=1), ones)
    ctx.close()
