"""GPU tests of the surface bounds (ocean_surface_bounds / _device, csrc/bounds.hip) and of the ray casts
(ocean_raycast / _device / _async, csrc/ray.hip).  The bounds are compared with numpy's min and max over the
read-back slices, the ray casts with restate_raycast (tests/test_ray_abi.py: numpy fp32 over oracle.sample_world,
every node of every ray evaluated, no air skip) applied to the context's own read-back textures.  Both
comparisons are bit for bit, with the air skip on and off."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_parity import _ctx_with_env
from test_gpu_query import Textures, make_ctx
from test_ray_abi import ray_positions, restate_raycast

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
STEPS, REFINE = 24, 8


def numpy_bounds(ctx, tile=0):
    d = ctx.read_all(oh.TEX_DISP, tile)
    return np.concatenate([d.min(axis=(1, 2)), d.max(axis=(1, 2))], axis=1)


def device_bounds(ctx, tile=0):
    import torch
    o = torch.zeros(ctx.C * 8, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ctx.surface_bounds_device(o.data_ptr(), tile)
    ctx.synchronize()
    return o.cpu().numpy().reshape(ctx.C, 8)


def skip_height(bounds):
    """The ray kernel's H (ray.hip), in its own fp32 operations: the cascade sum of max Dy plus 2^-19 times the
    cascade sum of max |Dy|."""
    top, mag = f32(0), f32(0)
    for lo, hi in zip(bounds[:, 1], bounds[:, 5]):
        top = top + hi
        mag = mag + max(abs(lo), abs(hi))
    return f32(top + mag * f32(2.0 ** -19))


def make_rays(bounds, m, seed):
    """The population of the issue, by construction, shuffled.  With H = the cascade sum of max |Dy|: a third from
    y in [1.5 H, 4 H] pointing down with t1 long enough to reach y = -2 H (a sign change: HIT), a third from the
    same heights pointing level or up (MISS), a sixth from below -1.5 H (SUBMERGED), and a sixth grazing: origins
    a few ulp around the kernel's skip height and around the sum of max Dy, slopes of a few degrees either way."""
    rng = np.random.default_rng(seed)
    H = float(np.maximum(np.abs(bounds[:, 1]), np.abs(bounds[:, 5])).astype(np.float64).sum())
    assert H > 0
    r = np.zeros((m, 8), f32)
    r[:, [0, 2]] = rng.uniform(-2000.0, 2000.0, (m, 2))
    kind = np.arange(m) % 6  # 0, 1: down; 2, 3: level or up; 4: below; 5: grazing
    down, up, below, graze = kind < 2, (kind == 2) | (kind == 3), kind == 4, kind == 5
    r[:, 1] = rng.uniform(1.5 * H, 4.0 * H, m)
    r[:, [3, 5]] = rng.uniform(-0.7, 0.7, (m, 2))
    r[down, 4] = -1.0
    r[down, 7] = (r[down, 1] + 2.0 * H) * 1.05
    r[up, 4] = np.where(rng.random(up.sum()) < 0.3, 0.0, rng.uniform(0.0, 1.0, up.sum()))
    r[up, 7] = rng.uniform(1.0, 200.0, up.sum())
    r[below, 1] = rng.uniform(-4.0 * H, -1.5 * H, below.sum())
    r[below, 4] = rng.uniform(-1.0, 1.0, below.sum())
    r[below, 7] = rng.uniform(1.0, 200.0, below.sum())
    g = np.flatnonzero(graze)
    hs, top = skip_height(bounds), f32(bounds[:, 5].sum(dtype=f32))
    base = np.where(np.arange(len(g)) % 2 == 0, hs, top).astype(f32)
    ulps = rng.integers(-2, 3, len(g)) * rng.choice([1, 16], len(g))
    r[g, 1] = base + ulps.astype(f32) * np.spacing(base)
    r[g, 3], r[g, 5] = np.cos(rng.uniform(0, 6.28, len(g))), np.sin(rng.uniform(0, 6.28, len(g)))
    r[g, 4] = np.tan(np.radians(rng.uniform(-5.0, 5.0, len(g))))
    r[g, 7] = rng.uniform(10.0, 400.0, len(g))
    r[g[::5], 6] = rng.uniform(-50.0, 0.0, len(g[::5]))  # a start behind the origin
    return np.ascontiguousarray(r[rng.permutation(m)])


# ---------------------------------------------------------------------------- bounds
@pytest.mark.parametrize("n,ncasc,tiles", [(16, 1, 1), (64, 4, 1), (256, 3, 2)])
def test_bounds_are_numpy_min_max(n, ncasc, tiles):
    """Exact: the records equal numpy's min / max over the read-back slices, for every tile, in both forms; after
    a second step (the cache was dropped), after ocean_write of a DISP slice with a planted extreme at the last
    texel, and after a device-side overwrite through the pointer of ocean_get_device_ptr (nothing cached)."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, times=(0.5,), tiles=tiles)
    for t in range(tiles):
        want = numpy_bounds(ctx, t)
        assert np.abs(want).max() > 0
        np.testing.assert_array_equal(ctx.surface_bounds(t), want)
        np.testing.assert_array_equal(ctx.surface_bounds(t), want)  # the cached answer
        np.testing.assert_array_equal(device_bounds(ctx, t), want)
    last = tiles - 1
    first = ctx.surface_bounds(last)
    ctx.step(1.0)
    got = ctx.surface_bounds(last)
    np.testing.assert_array_equal(got, numpy_bounds(ctx, last))
    assert not np.array_equal(got, first)  # the cached records of the first frame were dropped
    # a planted extreme at texel (N - 1, N - 1) of the last cascade's slice: the last texel the reduction reads
    sl = ctx.read(oh.TEX_DISP, last, ncasc - 1)
    sl[n - 1, n - 1] = [1.0e6, -2.0e6, 3.0e6, -4.0e6]
    ctx.write(oh.TEX_DISP, sl, last, ncasc - 1)
    got = ctx.surface_bounds(last)
    np.testing.assert_array_equal(got, numpy_bounds(ctx, last))
    np.testing.assert_array_equal(got[ncasc - 1, [4, 1, 6, 3]], f32([1.0e6, -2.0e6, 3.0e6, -4.0e6]))
    np.testing.assert_array_equal(device_bounds(ctx, last), got)
    # the pointer handed out: a foreign device-side write must be seen with no call on this context in between.
    # The writer is another context's kernel: its bounds record, (min xyzw, max xyzw) of a slice that is zero but
    # for one texel, lands on texels 0 and 1 of slice (last, 0) through the pointer.
    ptr, nbytes = ctx.device_ptr(oh.TEX_DISP)
    assert nbytes == tiles * ncasc * n * n * 16
    before = ctx.surface_bounds(last)
    w = make_ctx(16, O.SCENE_CASCADES[:1], times=())
    plant = np.zeros((16, 16, 4), f32)
    plant[5, 9] = [-7.0e6, 8.0e6, -9.0e6, 1.0e7]
    w.write(oh.TEX_DISP, plant)
    w.surface_bounds_device(ptr + last * ncasc * n * n * 16)
    w.synchronize()
    w.close()
    after = ctx.surface_bounds(last)
    np.testing.assert_array_equal(after, numpy_bounds(ctx, last))
    np.testing.assert_array_equal(after[0, [0, 5, 2, 7]], f32([-7.0e6, 8.0e6, -9.0e6, 1.0e7]))
    assert not np.array_equal(before, after)
    np.testing.assert_array_equal(device_bounds(ctx, last), after)
    ctx.close()


def test_bounds_errors():
    import torch
    ctx = oh.OceanContext(64, 2, 1)
    L, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    out = np.zeros((2, 8), f32)
    with pytest.raises(oh.OceanError) as e:
        ctx.surface_bounds()
    assert e.value.code == oh.E_STATE  # before ocean_init_spectrum
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    for tile, ptr, nbytes, word in ((1, out.ctypes.data, 64, b"tile"), (-1, out.ctypes.data, 64, b"tile"),
                                    (0, None, 64, b"output"), (0, out.ctypes.data, 32, b"byte"),
                                    (0, out.ctypes.data, 96, b"byte")):
        for fn in (L.ocean_surface_bounds, L.ocean_surface_bounds_device):
            assert fn(h, tile, vp(ptr) if ptr else None, nbytes) == oh.E_INVALID_ARG
            assert word in L.ocean_last_error()
    o = torch.zeros(20, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    assert L.ocean_surface_bounds_device(h, 0, vp(o.data_ptr() + 4), 64) == oh.E_INVALID_ARG
    assert b"aligned" in L.ocean_last_error()
    np.testing.assert_array_equal(ctx.surface_bounds(), np.zeros((2, 8), f32))  # no frame yet: DISP is zero
    ctx.close()
    # a column band is allowed: the columns the context does not write are zero and take part
    band = make_ctx(512, O.SCENE_CASCADES[:1], times=(0.5,))
    whole = band.surface_bounds()
    band.set_column_band(0, 256)
    band.step(1.0)
    got = band.surface_bounds()
    np.testing.assert_array_equal(got, numpy_bounds(band))
    assert not np.array_equal(got, whole)
    band.close()
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    with pytest.raises(oh.OceanError) as e:
        par.surface_bounds()
    assert e.value.code == oh.E_UNSUPPORTED
    with pytest.raises(oh.OceanError) as e:
        par.raycast(np.zeros((1, 8), f32))
    assert e.value.code == oh.E_UNSUPPORTED
    with pytest.raises(oh.OceanError) as e:
        par.raycast_async(np.zeros((1, 8), f32))
    assert e.value.code == oh.E_UNSUPPORTED
    par.close()


# ---------------------------------------------------------------------------- ray casts
def check_population(status, m):
    for s, name in ((oh.RAY_MISS, "MISS"), (oh.RAY_HIT, "HIT"), (oh.RAY_SUBMERGED, "SUBMERGED")):
        share = (status == s).sum() / m
        print(f"{name}: {share:.3f} of {m} rays")
        assert share >= 0.1, name


@pytest.mark.parametrize("n,ncasc,flags", [(64, 1, 0), (64, 4, 0), (128, 2, oh.F_MIPS),
                                           (64, 3, oh.F_DISPLACEMENT_ONLY)])
def test_raycast_matches_restatement(n, ncasc, flags):
    """Bit for bit against the restatement: 2048 + 37 rays, count = 1 and count = 256, K in {0, 2}, S = 24, B = 8 and
    once B = 0.  The (64, 4) scene folds (its 34 m cascade is not contractive at 64^2) and must match all the same,
    with finite output.  The statuses the construction guarantees are checked on their own."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = Textures(ctx, cas)
    m = 2048 + 37
    rays = make_rays(ctx.surface_bounds(), m, n + ncasc)
    for k, refine in ((0, REFINE), (2, REFINE), (2, 0)):
        want = restate_raycast(tex, rays, k, STEPS, refine)
        got = ctx.raycast(rays, iterations=k, steps=STEPS, refine=refine)
        assert np.isfinite(got).all()
        np.testing.assert_array_equal(got, want, err_msg=f"K = {k}, B = {refine}")
        check_population(got[:, 3], m)
        for count in (1, 256):
            np.testing.assert_array_equal(ctx.raycast(rays[:count], iterations=k, steps=STEPS, refine=refine),
                                          want[:count])
    # by construction: down from above hits, level or up misses, from below is submerged
    got = ctx.raycast(rays, iterations=2, steps=STEPS, refine=REFINE)
    H = float(np.abs(tex.disp[..., 1]).max(axis=(1, 2)).sum())
    high, t0 = rays[:, 1] >= 1.5 * H, rays[:, 6] == 0
    np.testing.assert_array_equal(got[high & t0 & (rays[:, 4] == -1), 3], oh.RAY_HIT)
    np.testing.assert_array_equal(got[high & t0 & (rays[:, 4] >= 0), 3], oh.RAY_MISS)
    np.testing.assert_array_equal(got[(rays[:, 1] <= -1.5 * H), 3], oh.RAY_SUBMERGED)
    if flags & oh.F_DISPLACEMENT_ONLY:
        np.testing.assert_array_equal(got[:, 4:], np.tile(f32([0, 1, 0, 0]), (m, 1)))
    np.testing.assert_array_equal(ctx.raycast(rays[:256]), restate_raycast(tex, rays[:256], 4, 64, 8))  # the defaults
    ctx.close()


def test_air_skip_changes_no_bit_and_bounds_run_once_per_frame():
    """OCEAN_RAY_BOUNDS=0 and =1 give identical arrays, both the restatement's.  With the skip on, two ray casts in
    one frame launch the bounds kernels once (kind 2: one bounds entry and two ray entries), a new frame launches
    them again, and with the skip off a ray cast launches none."""
    n, cas = 64, O.SCENE_CASCADES[:3]
    on, _ = _ctx_with_env({"OCEAN_RAY_BOUNDS": "1"}, n, cas)
    off, _ = _ctx_with_env({"OCEAN_RAY_BOUNDS": "0"}, n, cas)
    for ctx in (on, off):
        ctx.step(0.5)
        ctx.step(1.0)
    tex = Textures(on, cas)
    np.testing.assert_array_equal(off.read_all(oh.TEX_DISP), tex.disp)
    rays = make_rays(on.surface_bounds(), 2048 + 37, 3)
    want = restate_raycast(tex, rays, 2, STEPS, REFINE)
    a = on.raycast(rays, iterations=2, steps=STEPS, refine=REFINE)
    b = off.raycast(rays, iterations=2, steps=STEPS, refine=REFINE)
    np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(a, want)
    check_population(a[:, 3], len(rays))
    for ctx, launches, skip in ((on, 3, True), (off, 2, False)):
        ctx.set_kernel_timing(True)
        ctx.step(1.5)
        ctx.kernel_stats(2)  # (reset: the frame itself may count kind-2 launches)
        ctx.raycast(rays[:256], iterations=2, steps=STEPS, refine=REFINE)
        ctx.raycast(rays[:256], iterations=2, steps=STEPS, refine=REFINE)
        ms, count = ctx.kernel_stats(2)
        assert count == launches and ms > 0, (count, launches)
        assert "k_raycast" in ctx.kernel_name(2)
        ctx.surface_bounds()  # cached where the skip computed it; the first computation of this frame otherwise
        ms, count = ctx.kernel_stats(2)
        assert count == (0 if skip else 1)
        if not skip:
            assert "k_bounds_reduce" in ctx.kernel_name(2)
        ctx.step(2.0)
        ctx.kernel_stats(2)
        ctx.raycast(rays[:1], iterations=0, steps=1, refine=0)
        assert ctx.kernel_stats(2)[1] == (2 if skip else 1)  # a new frame: the bounds again
        ctx.set_kernel_timing(False)
    on.close()
    off.close()


def test_raycast_is_consistent_with_the_queries():
    """For HIT rays out[1] <= 0, and the record's tail is what ocean_query_surface returns for o + t* d.  S = 1,
    B = 0 reduces to two queries: the sign of f at t0 and at t1 decides, from ocean_query_surface's own heights."""
    n, cas, k = 64, O.SCENE_CASCADES[:2], 2
    ctx = make_ctx(n, cas)
    rays = make_rays(ctx.surface_bounds(), 1024, 9)
    got = ctx.raycast(rays, iterations=k, steps=STEPS, refine=REFINE)
    hit = got[:, 3] == oh.RAY_HIT
    assert hit.sum() > 100 and (got[hit, 1] <= 0).all()
    pos = ray_positions(rays, got[:, 0])
    rec = ctx.query_surface(np.ascontiguousarray(pos[:, [0, 2]]), iterations=k)
    np.testing.assert_array_equal(got[:, 1], pos[:, 1] - rec[:, 0])
    np.testing.assert_array_equal(got[:, 2], rec[:, 3])
    np.testing.assert_array_equal(got[:, 4:], rec[:, 4:])
    one = ctx.raycast(rays, iterations=k, steps=1, refine=0)
    t0, ts = rays[:, 6], rays[:, 6] + (rays[:, 7] - rays[:, 6])  # t_S = t0 + 1 * dt, dt = (t1 - t0) / 1
    p0, p1 = ray_positions(rays, t0), ray_positions(rays, ts)
    f0 = p0[:, 1] - ctx.query_surface(np.ascontiguousarray(p0[:, [0, 2]]), iterations=k)[:, 0]
    f1 = p1[:, 1] - ctx.query_surface(np.ascontiguousarray(p1[:, [0, 2]]), iterations=k)[:, 0]
    status = np.where(~(f0 > 0), oh.RAY_SUBMERGED, np.where(~(f1 > 0), oh.RAY_HIT, oh.RAY_MISS))
    np.testing.assert_array_equal(one[:, 3], status)
    np.testing.assert_array_equal(one[:, 0], np.where(~(f0 > 0), t0, ts))
    np.testing.assert_array_equal(one[:, 1], np.where(~(f0 > 0), f0, f1))
    ctx.close()


def test_raycast_forms_agree_and_async_snapshots_behind_later_steps():
    """The three forms agree; the async request made after step t1, with two more steps queued right behind it,
    holds the answer of t1 (a second context gives it), and the caller's rays, overwritten right after the call,
    are not read again."""
    import torch
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
    ref.step(times[0])
    rays = make_rays(ref.surface_bounds(), 1000, 5)
    buf = rays.copy()
    ctx.step(times[0])
    rb = ctx.raycast_async(buf, iterations=2, steps=STEPS, refine=REFINE)
    buf[:] = 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    rb.release()
    want = ref.raycast(rays, iterations=2, steps=STEPS, refine=REFINE)
    np.testing.assert_array_equal(got, want)
    later = ctx.raycast(rays, iterations=2, steps=STEPS, refine=REFINE)  # the blocking form now: frame t3
    assert not np.array_equal(got[:, 0], later[:, 0])
    slot = oh.PinnedBuffer(len(rays) * 32)
    rb = ctx.raycast_async(rays, iterations=2, steps=STEPS, refine=REFINE, buf=slot)
    np.testing.assert_array_equal(rb.data, later)
    rb.release()
    slot.release()
    # the device form: async on the ctx stream; misaligned pointers are refused, not faulted on
    dev = torch.device("cuda", ctx.device)
    m = len(rays)
    r = torch.zeros(m * 8 + 1, dtype=torch.float32, device=dev)
    r[:m * 8] = torch.from_numpy(rays.ravel()).to(dev)
    o = torch.zeros(m * 8 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.raycast_device(r.data_ptr(), m, o.data_ptr(), iterations=2, steps=STEPS, refine=REFINE)
    L, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    assert L.ocean_raycast_device(h, 0, 2, STEPS, REFINE, vp(r.data_ptr() + 2), m, vp(o.data_ptr())) == oh.E_INVALID_ARG
    assert L.ocean_raycast_device(h, 0, 2, STEPS, REFINE, vp(r.data_ptr()), m, vp(o.data_ptr() + 4)) == oh.E_INVALID_ARG
    assert b"aligned" in L.ocean_last_error()
    assert L.ocean_raycast_device(h, 0, 2, STEPS, REFINE, vp(r.data_ptr()), 0, vp(o.data_ptr())) == oh.OK
    ctx.synchronize()
    np.testing.assert_array_equal(o[:m * 8].cpu().numpy().reshape(m, 8), later)
    # rays 4-byte aligned only: a device array that starts one float in
    r2 = torch.zeros(m * 8 + 1, dtype=torch.float32, device=dev)
    r2[1:] = torch.from_numpy(rays.ravel()).to(dev)
    torch.cuda.synchronize()
    ctx.raycast_device(r2.data_ptr() + 4, m, o.data_ptr(), iterations=2, steps=STEPS, refine=REFINE)
    ctx.synchronize()
    np.testing.assert_array_equal(o[:m * 8].cpu().numpy().reshape(m, 8), later)
    ctx.close()
    ref.close()


def test_raycast_errors():
    """Every error of the validation list returns its code and ocean_last_error names the argument; *req is NULL
    after every failure."""
    rays = np.zeros((8, 8), f32)
    rays[:, 1], rays[:, 4], rays[:, 7] = 50.0, -1.0, 100.0
    ctx = oh.OceanContext(64, 2, 1)
    for call in (ctx.raycast, ctx.raycast_async):
        with pytest.raises(oh.OceanError) as e:
            call(rays)
        assert e.value.code == oh.E_STATE and "ocean_init_spectrum" in str(e.value)  # before ocean_init_spectrum
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    bad = [(dict(tile=1), "tile"), (dict(tile=-1), "tile"), (dict(iterations=17), "iterations"),
           (dict(iterations=-1), "iterations"), (dict(steps=0), "steps"), (dict(steps=oh.RAY_MAX_STEPS + 1), "steps"),
           (dict(refine=-1), "refine"), (dict(refine=33), "refine")]
    for kw, word in bad:
        for call in (ctx.raycast, ctx.raycast_async):
            with pytest.raises(oh.OceanError) as e:
                call(rays, **kw)
            assert e.value.code == oh.E_INVALID_ARG and word in str(e.value), kw
    L, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    out = np.zeros((8, 8), f32)
    req = ctypes.c_void_p(0x1234)
    for fn, extra in ((L.ocean_raycast, ()), (L.ocean_raycast_device, ()), (L.ocean_raycast_async, (ctypes.byref(req),))):
        for r_, o_, count, word in ((None, out.ctypes.data, 8, b"null"), (rays.ctypes.data, None, 8, b"null"),
                                    (rays.ctypes.data, out.ctypes.data, -1, b"negative")):
            req.value = 0x1234
            assert fn(h, 0, 4, 16, 8, vp(r_) if r_ else None, count, vp(o_) if o_ else None, *extra) == oh.E_INVALID_ARG
            assert word in L.ocean_last_error()
            assert not extra or req.value is None
    assert L.ocean_raycast_async(h, 0, 4, 16, 8, vp(rays.ctypes.data), 8, vp(out.ctypes.data), None) == oh.E_INVALID_ARG
    assert b"req" in L.ocean_last_error()
    many = np.zeros((oh.RAY_MAX_RAYS + 1, 8), f32)
    for call in (ctx.raycast, ctx.raycast_async):
        with pytest.raises(oh.OceanError) as e:
            call(many, steps=4)
        assert e.value.code == oh.E_INVALID_ARG and "OCEAN_RAY_MAX_RAYS" in str(e.value)
    # count * steps in 64 bits: the host forms cannot exceed it (16384 x 1024 = 2^24); the device form can, and
    # 2^22 rays of 1024 steps = 2^32 samples are refused before any device call (the pointers are never read)
    for count in (oh.RAY_MAX_RAYS + 1, 1 << 22):
        assert L.ocean_raycast_device(h, 0, 0, 1024, 0, vp(rays.ctypes.data), count, vp(out.ctypes.data)) == oh.E_INVALID_ARG
        assert b"OCEAN_RAY_MAX_SAMPLES" in L.ocean_last_error()
    assert ctx.raycast(many[:-1], steps=2, refine=0).shape == (oh.RAY_MAX_RAYS, 8)  # the maximum itself is served
    assert ctx.raycast(np.zeros((0, 8), f32)).shape == (0, 8)  # count 0: a no-op
    with pytest.raises(oh.OceanError) as e:
        ctx.raycast_async(np.zeros((0, 8), f32))  # ... but no request to hand back
    assert e.value.code == oh.E_INVALID_ARG
    ctx.close()


def test_raycast_and_bounds_on_a_later_tile():
    """T = 3: tile 2's rays and bounds are checked against tile 2's own textures, and tile 0's answers differ."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, tiles=3)
    b2 = ctx.surface_bounds(2)
    np.testing.assert_array_equal(b2, numpy_bounds(ctx, 2))
    assert not np.array_equal(b2, ctx.surface_bounds(0))
    rays = make_rays(b2, 600, 21)
    got = ctx.raycast(rays, tile=2, iterations=2, steps=STEPS, refine=REFINE)
    np.testing.assert_array_equal(got, restate_raycast(Textures(ctx, cas, tile=2), rays, 2, STEPS, REFINE))
    other = ctx.raycast(rays, tile=0, iterations=2, steps=STEPS, refine=REFINE)
    np.testing.assert_array_equal(other, restate_raycast(Textures(ctx, cas, tile=0), rays, 2, STEPS, REFINE))
    assert not np.array_equal(got, other)
    rb = ctx.raycast_async(rays, tile=2, iterations=2, steps=STEPS, refine=REFINE)
    np.testing.assert_array_equal(rb.data, got)
    rb.release()
    ctx.close()


def test_water_body_raycast_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    wb.Update(0.5)
    hit = wb.Raycast((3.0, 30.0, -4.0), (0.0, -2.0, 0.0), 60.0)
    ray = f32([[3.0, 30.0, -4.0, 0.0, -1.0, 0.0, 0.0, 60.0]])
    rec = wb.ctx.raycast(ray)[0]
    assert hit is not None and not hit.submerged and rec[3] == oh.RAY_HIT
    assert hit.distance == rec[0] and hit.foam == rec[7]
    np.testing.assert_array_equal(hit.normal, rec[4:7])
    np.testing.assert_array_equal(hit.point, ray[0, :3] + rec[0] * ray[0, 3:6])
    assert wb.Raycast((3.0, 30.0, -4.0), (0.0, 1.0, 0.0), 60.0) is None
    assert wb.Raycast((3.0, -30.0, -4.0), (0.0, 1.0, 0.0), 10.0).submerged
    rec = wb.ctx.surface_bounds()
    np.testing.assert_array_equal(wb.SurfaceBounds(), np.stack([rec[:, 0:3].sum(axis=0, dtype=f32),
                                                                rec[:, 4:7].sum(axis=0, dtype=f32)]))
    wb.OnDisable()
