"""GPU tests of the surface queries (ocean_query_surface / _device / _async, csrc/query.hip) and of the
facades' readback "probes".  The query is restated here in numpy fp32 on top of oracle.sample_world with
lod 0 (the same operations in the same order, include/ocean/ocean.h), applied to the context's own
read-back textures: the comparison is bit for bit."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_sample import _points

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
EPS32 = float(np.finfo(np.float32).eps)


class Textures:
    """The context's own DISP / DERIV / TURB of tile `tile`, read back once, and S(p) over them."""

    def __init__(self, ctx, cas, tile=0):
        full = not ctx.flags & oh.F_DISPLACEMENT_ONLY
        self.lengths = [c["wavelength"] for c in cas]
        self.disp = ctx.read_all(oh.TEX_DISP, tile)
        self.deriv = ctx.read_all(oh.TEX_DERIV, tile) if full else None
        self.turb = ctx.read_all(oh.TEX_TURB, tile) if full else None

    def _pts(self, p):
        return np.concatenate([p, np.zeros((len(p), 1), f32)], axis=1)  # lod 0: level 0 also with mip chains

    def S(self, p):
        return O.sample_world(self.disp, self.deriv, self.turb, self.lengths, self._pts(p))

    def S_disp(self, p):  # the DISP taps alone: the same bits as S(p)[:, 0, :3]
        return O.sample_world(self.disp, None, None, self.lengths, self._pts(p))[:, 0]


def restate_surface(tex, q, ks):
    """OCEAN_QUERY_SURFACE for every K in `ks` (ascending), in one pass over the iteration: {K: [M][8]}."""
    q = np.asarray(q, f32)
    p = q.copy()
    out = {}
    for k in range(max(ks) + 1):
        if k in ks:
            s = tex.S(p)
            d = s[:, 0]
            r = np.maximum(np.abs((p[:, 0] + d[:, 0]) - q[:, 0]), np.abs((p[:, 1] + d[:, 2]) - q[:, 1]))
            out[k] = np.stack([d[:, 1], p[:, 0], p[:, 1], r, s[:, 2, 0], s[:, 2, 1], s[:, 2, 2], s[:, 0, 3]], axis=1)
        d = tex.S_disp(p)
        p = np.stack([q[:, 0] - d[:, 0], q[:, 1] - d[:, 2]], axis=1)
    return out


def restate_reference(disp0, q):
    """OCEAN_QUERY_REFERENCE: GetWaterHeight's texel pick (WaterBody.cs:195-209) in fp32; disp0 = slice 0."""
    n = disp0.shape[0]
    a, b = f32(-(n // 2)), f32(n // 2)

    def texel(w):
        u = np.minimum(np.maximum((np.asarray(w, f32) - a) / (b - a), f32(0)), f32(1))
        return np.clip((u * f32(n)).astype(np.int64), 0, n - 1)

    px, py = texel(q[:, 0]), texel(q[:, 1])
    out = np.zeros((len(q), 8), f32)
    out[:, 0], out[:, 1], out[:, 2] = disp0[py, px, 1], px, py
    return out


def make_ctx(n, cas, flags=0, noise=None, times=(0.5, 1.0), tiles=1):
    ctx = oh.OceanContext(n, len(cas), tiles, flags)
    ctx.set_params(O.scene_params(), cas)
    for t in range(tiles):  # its own noise per tile, so that no two tiles hold the same water
        ctx.set_noise(t, O.generate_noise(n, 20251121 + t) if noise is None else noise)
    ctx.init_spectrum()
    for t in times:
        ctx.step(t)
    return ctx


KS = (0, 1, 4, 16)


@pytest.mark.parametrize("n,ncasc,flags", [(64, 1, 0), (64, 4, 0), (256, 3, oh.F_DISPLACEMENT_ONLY),
                                           (128, 2, oh.F_MIPS)])
def test_query_matches_restatement_and_sample_world(n, ncasc, flags):
    """Bit-exact against the restatement for K in {0, 1, 4, 16}; the (64, 4) scene is not contractive (its
    34 m cascade folds at 64^2) and must match bit for bit all the same, with finite output.  Consistency
    with ocean_sample_world: K = 0 is the sample at q, and the K = 4 answer is the sample at its own p_K."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    q = np.ascontiguousarray(_points(4096, n, n + ncasc)[:, :2])
    tex = Textures(ctx, cas)
    want = restate_surface(tex, q, KS)
    got = {}
    for k in KS:
        got[k] = ctx.query_surface(q, iterations=k)
        assert np.isfinite(got[k]).all()
        np.testing.assert_array_equal(got[k], want[k], err_msg=f"K = {k}")
    np.testing.assert_array_equal(got[0][:, 1:3], q)  # p_0 = q
    for k, p in ((0, q), (4, got[4][:, 1:3])):
        s = ctx.sample_world(np.concatenate([p, np.zeros((len(p), 1), f32)], axis=1))
        np.testing.assert_array_equal(got[k][:, 0], s[:, 0, 1])    # height
        np.testing.assert_array_equal(got[k][:, 4:7], s[:, 2, :3])  # normal
        np.testing.assert_array_equal(got[k][:, 7], s[:, 0, 3])    # foam
    if flags & oh.F_DISPLACEMENT_ONLY:
        np.testing.assert_array_equal(got[4][:, 4:], np.tile(f32([0, 1, 0, 0]), (len(q), 1)))
    # the default arguments: surface mode, 4 steps
    np.testing.assert_array_equal(ctx.query_surface(q), got[4])
    ctx.close()


def test_query_converges_by_the_derived_bound():
    """The fixed point contracts at the rate the displacement's Lipschitz constant gives.  D(p) = sum_c
    bilinear(DISP_c)(p / L_c): a bilinear patch's slope along x is at most the largest difference of x
    neighbours times the N / L_c texels per metre, so in the max norm |D_xz(p) - D_xz(p')| <= l |p - p'| with
    l = sum_c (N / L_c) (max |d_x D_xz| + max |d_y D_xz|), wrapped differences, the max over texels and both
    components.  One step's residual is the previous step's displacement difference: p_K + D(p_K) - q =
    D(p_K) - D(p_{K-1}) and p_K - p_{K-1} = -(p_{K-1} + D(p_{K-1}) - q), so r_K <= l r_{K-1} up to the
    roundings of p_K, of the sample positions and of r itself, each a few ulp of |q| or |D|: 8 eps (|q| + |D|).
    On the CPU oracle this scene gives l = 0.239 and max |D_xz| = 1.12 m."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, noise=O.generate_noise(n, 7))
    disp = ctx.read_all(oh.TEX_DISP)
    ell, dmax = 0.0, 0.0
    for c, cc in enumerate(cas):
        dxz = disp[c][..., [0, 2]].astype(np.float64)
        ddx = np.abs(np.roll(dxz, -1, axis=1) - dxz).max()
        ddy = np.abs(np.roll(dxz, -1, axis=0) - dxz).max()
        ell += n / cc["wavelength"] * (ddx + ddy)
        dmax += np.abs(dxz).max()
    print(f"l = {ell:.4f}, sum_c max|D_xz| = {dmax:.4f}")
    assert ell <= 0.5
    rng = np.random.default_rng(11)
    q = rng.uniform(-2000.0, 2000.0, (4096, 2)).astype(f32)
    r = [ctx.query_surface(q, iterations=k)[:, 3].astype(np.float64) for k in range(7)]
    slack = 8 * EPS32 * (np.abs(q).max(axis=1).astype(np.float64) + dmax)
    for k in range(1, 7):
        print(f"K = {k}: max r = {r[k].max():.3e}, max (r_K - l r_(K-1)) / slack = "
              f"{((r[k] - ell * r[k - 1]) / slack).max():.3f}")
        assert (r[k] <= ell * r[k - 1] + slack).all(), f"K = {k}"
    print(f"max r_0 = {r[0].max():.4f}, max r_4 = {r[4].max():.3e}")
    assert r[4].max() < r[0].max() / 50  # the iterations demonstrably do something
    ctx.close()


def test_query_flat_sea_known_answer():
    """Zero noise: no waves.  Height 0, p = q, r = 0 and the normal (0, 1, 0) at every K."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, noise=np.zeros((n, n, 2), f32))
    q = np.ascontiguousarray(_points(512, n, 3)[:, :2])
    for k in (0, 4):
        got = ctx.query_surface(q, iterations=k)
        want = np.zeros((len(q), 7), f32)
        want[:, 1:3] = q
        want[:, 5] = 1.0
        np.testing.assert_array_equal(got[:, :7], want)
    ctx.close()


def test_query_reference_mode_is_get_water_height():
    """OCEAN_QUERY_REFERENCE against WaterBody.GetWaterHeight over a landed "height" readback of the same
    frame, bitwise.  The points -- integers + {0, 0.25, 0.5} across [-N/2 - 3, N/2 + 3] on both axes -- are
    exactly representable, so the reference's double arithmetic and the kernel's fp32 agree; both ends clamp."""
    n = 64
    wb = oh.scene_water_body(n=n, n_cascades=2, readback="height").Awake()
    wb.Update(0.5)
    wb.Update(1.0)
    wb.WaitForReadback()
    axis = np.concatenate([np.arange(-n // 2 - 3, n // 2 + 4) + fr for fr in (0.0, 0.25, 0.5)]).astype(f32)
    axis = axis[axis <= n // 2 + 3]
    xs, zs = np.meshgrid(axis, axis[::-1], indexing="xy")
    q = np.stack([xs.ravel(), zs.ravel()], axis=1)
    assert len(q) <= oh.QUERY_MAX_POINTS
    got = wb.ctx.query_surface(q, mode=oh.QUERY_REFERENCE, iterations=0)
    want = restate_reference(wb.ctx.read(oh.TEX_DISP, 0, 0), q)
    np.testing.assert_array_equal(got, want)
    heights = f32([wb.GetWaterHeight((x, 0.0, z)) for x, z in q])
    np.testing.assert_array_equal(got[:, 0], heights)
    # the expected texels, written out: world w -> clamp(int((w + N/2) / N * N)) = clamp(floor(w) + N/2)
    np.testing.assert_array_equal(got[:, 1], np.clip(np.floor(q[:, 0]) + n // 2, 0, n - 1))
    np.testing.assert_array_equal(got[:, 2], np.clip(np.floor(q[:, 1]) + n // 2, 0, n - 1))
    assert (q[:, 0] < -n // 2).any() and (q[:, 0] > n // 2).any()  # clamped at both ends
    assert got[:, 1].min() == 0 and got[:, 1].max() == n - 1 and got[:, 2].min() == 0 and got[:, 2].max() == n - 1
    wb.OnDisable()


def test_query_async_snapshots_behind_later_steps():
    """ocean_query_surface_async: the request made after step t1, with two more steps queued right behind it,
    holds the answer of t1 (a second context gives it), and the caller's points buffer, overwritten right
    after the call, is not read again."""
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
    q = np.ascontiguousarray(_points(1000, n, 5)[:, :2])
    buf = q.copy()
    ctx.step(times[0])
    rb = ctx.query_surface_async(buf)
    buf[:] = 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    rb.release()
    ref.step(times[0])
    np.testing.assert_array_equal(got, ref.query_surface(q))
    later = ctx.query_surface(q)  # the blocking query now: frame t3
    assert not np.array_equal(got[:, 0], later[:, 0])
    # a reference-mode request through the same path, and a caller-owned pinned slot
    slot = oh.PinnedBuffer(len(q) * 32)
    rb = ctx.query_surface_async(q, mode=oh.QUERY_REFERENCE, iterations=0, buf=slot)
    np.testing.assert_array_equal(rb.data, ctx.query_surface(q, mode=oh.QUERY_REFERENCE, iterations=0))
    rb.release()
    slot.release()
    ctx.close()
    ref.close()


def test_query_errors_and_device_form():
    import torch
    pts = np.zeros((8, 2), f32)
    ctx = oh.OceanContext(64, 2, 1)
    with pytest.raises(oh.OceanError) as e:
        ctx.query_surface(pts)
    assert e.value.code == oh.E_STATE  # before ocean_init_spectrum
    with pytest.raises(oh.OceanError) as e:
        ctx.query_surface_async(pts)
    assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    bad = [dict(tile=1), dict(tile=-1), dict(mode=2), dict(mode=-1), dict(iterations=17), dict(iterations=-1),
           dict(mode=oh.QUERY_REFERENCE, iterations=1)]
    for kw in bad:
        for call in (ctx.query_surface, ctx.query_surface_async):
            with pytest.raises(oh.OceanError) as e:
                call(pts, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
    many = np.zeros((oh.QUERY_MAX_POINTS + 1, 2), f32)
    for call in (ctx.query_surface, ctx.query_surface_async):
        with pytest.raises(oh.OceanError) as e:
            call(many)
        assert e.value.code == oh.E_INVALID_ARG
    assert ctx.query_surface(many[:-1]).shape == (oh.QUERY_MAX_POINTS, 8)  # the maximum itself is served
    assert ctx.query_surface(np.zeros((0, 2), f32)).shape == (0, 8)  # count 0: a no-op
    with pytest.raises(oh.OceanError) as e:
        ctx.query_surface_async(np.zeros((0, 2), f32))  # ... but no request to hand back
    assert e.value.code == oh.E_INVALID_ARG
    # the device form: async on the ctx stream, and misaligned pointers are refused, not faulted on
    dev = torch.device("cuda", ctx.device)
    q = np.ascontiguousarray(_points(8, 64, 1)[:, :2])
    p = torch.zeros(8 * 2 + 1, dtype=torch.float32, device=dev)
    p[:16] = torch.from_numpy(q.ravel()).to(dev)
    o = torch.zeros(8 * 8 + 4, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    lib, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    assert lib.ocean_query_surface_device(h, 0, oh.QUERY_SURFACE, 4, vp(p.data_ptr()), 8, vp(o.data_ptr())) == oh.OK
    assert lib.ocean_query_surface_device(h, 0, oh.QUERY_SURFACE, 4, vp(p.data_ptr() + 2), 8,
                                          vp(o.data_ptr())) == oh.E_INVALID_ARG
    assert lib.ocean_query_surface_device(h, 0, oh.QUERY_SURFACE, 4, vp(p.data_ptr()), 8,
                                          vp(o.data_ptr() + 4)) == oh.E_INVALID_ARG
    assert lib.ocean_query_surface_device(h, 0, oh.QUERY_SURFACE, 4, vp(p.data_ptr()), 0, vp(o.data_ptr())) == oh.OK
    ctx.synchronize()
    np.testing.assert_array_equal(o[:64].cpu().numpy().reshape(8, 8), ctx.query_surface(q))
    ctx.close()
    # a column-parity shard holds half the columns: unsupported, as world sampling
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    for call in (par.query_surface, par.query_surface_async):
        with pytest.raises(oh.OceanError) as e:
            call(pts)
        assert e.value.code == oh.E_UNSUPPORTED
    par.close()


def test_water_body_probes_loop():
    """readback "probes": 6 Updates with 5 probes.  After WaitForReadback, ProbeHeights is the blocking query
    at the last frame; each earlier landed array is the answer of some frame k <= f, k monotone (requests
    complete in order; the acceptance of tests/test_gpu_host.py).  GetWaterHeight keeps returning 0."""
    n, C, F = 256, 3, 6
    bodies = f32([[0.0, 0.0, 0.0], [37.5, 1.0, -12.25], [-410.0, 0.0, 250.75], [1e4, -2.0, -3333.0], [-0.5, 0.0, n]])
    wb = oh.scene_water_body(n=n, n_cascades=C, readback="probes", probeCapacity=5)
    wb.SetProbes(bodies)
    wb.Awake()
    ref = oh.OceanContext(n, C, 1, oh.F_MIPS)
    ref.set_params(wb.params(), [c.as_dict() for c in wb.cascades])
    ref.generate_noise(wb.seed)
    ref.init_spectrum()
    q = np.ascontiguousarray(bodies[:, [0, 2]])
    assert wb.ProbeHeights is None
    seen, frames = [], []
    for f in range(F):
        wb.Update(f / 60.0)
        seen.append(wb.ProbeHeights)
        ref.step(f / 60.0)
        frames.append(ref.query_surface(q))
    wb.WaitForReadback()
    np.testing.assert_array_equal(wb.ProbeHeights, frames[-1][:, 0])
    np.testing.assert_array_equal(wb.ProbeResults, frames[-1])
    np.testing.assert_array_equal(wb.ProbeResults, wb.ctx.query_surface(q))
    last = -1
    for f in range(F):
        if seen[f] is None:
            assert last == -1, f"frame {f}: no answer after one had landed"
            continue
        cands = [k for k in range(f + 1) if np.array_equal(seen[f], frames[k][:, 0])]
        assert cands, f"frame {f}: heights match no completed frame"
        assert max(cands) >= last
        last = max(cands)
    assert wb.GetWaterHeight((0.0, 0.0, 0.0)) == 0.0 and wb.buoyancyData is None
    # reference mode through the facade, and fewer probes than the ring holds
    wb.probeMode, wb.probeIterations = oh.QUERY_REFERENCE, 0
    wb.SetProbes(bodies[:3])
    wb.Update(F / 60.0)
    wb.WaitForReadback()
    np.testing.assert_array_equal(wb.ProbeResults, wb.ctx.query_surface(q[:3], mode=oh.QUERY_REFERENCE, iterations=0))
    wb.OnDisable()
    assert wb.ProbeHeights.shape == (3,)  # the last answer outlives the pinned ring
    ref.close()
