"""GPU tests of the camera views (ocean_camera / _device / _async, csrc/view.hip) against restate_camera
(tests/test_camera_abi.py: numpy fp32 over restate_raycast and oracle.sample_world) applied to the context's own
read-back textures.  The ray records and the range image are compared bit for bit, also with ocean_raycast on the
same context over the restatement's rays; the colours against a float64 evaluation of the same formulas, by the
yardstick of the fp32 restatement's own rounding.

The image is 45 x 37 (a multiple of no tile shape: both tail edges have partial tiles), S = 32, B = 6, K = 2.  The
poses were chosen on the CPU over the oracle's textures of the same scenes so that the horizon crosses the image:
pose_above sits a few metres over the highest crest the bounds allow and sees water in the lower rows and sky in
the upper ones; pose_below sits under the lowest trough.  Each test asserts the shares on the restatement."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_camera_abi import camera_rays, colours, restate_camera, shading_inputs
from test_gpu_parity import _ctx_with_env
from test_gpu_query import Textures, make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
W, H, K, STEPS, REFINE = 45, 37, 2, 32, 6
CONTEXTS = [(64, 1, 0), (64, 4, 0), (128, 2, oh.F_MIPS), (64, 2, oh.F_DISPLACEMENT_ONLY)]


def pose_above(bounds):
    """Four metres over the cascade sum of max y, looking 8 degrees below the level over 400 m."""
    top = float(bounds[:, 5].astype(np.float64).sum())
    eye = np.float64([3.0, top + 4.0, -4.0])
    ahead = np.float64([0.6, 0.0, 0.8])
    target = eye + 100.0 * ahead + np.float64([0.0, -100.0 * np.tan(np.radians(8.0)), 0.0])
    return oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 0.9, W, H, 0.0, 400.0)


def pose_below(bounds):
    """Three metres under the cascade sum of min y, looking up and ahead: every pixel starts under water."""
    low = float(bounds[:, 1].astype(np.float64).sum())
    eye = np.float64([-7.0, low - 3.0, 11.0])
    return oh.look_at_camera(eye, eye + np.float64([0.5, 0.4, -0.7]), (0.0, 1.0, 0.0), 0.9, W, H, 0.0, 50.0)


def mip_textures(ctx, cas, tile=0):
    """Textures with the context's mip chains beside them, for the restatement's samples at a lod."""
    tex = Textures(ctx, cas, tile)
    if ctx.flags & oh.F_MIPS:
        levels = range(1, int(np.log2(ctx.n)) + 1)
        tex.deriv_mips = [[ctx.read_mip(oh.TEX_DERIV, lv, tile, c) for lv in levels] for c in range(len(cas))]
        tex.turb_mips = [[ctx.read_mip(oh.TEX_TURB, lv, tile, c) for lv in levels] for c in range(len(cas))]
    return tex


def check_shares(status):
    hit, miss = (status == oh.RAY_HIT).mean(), (status == oh.RAY_MISS).mean()
    print(f"hit {hit:.3f}, miss {miss:.3f} of {len(status)} pixels")
    assert hit >= 0.2 and miss >= 0.1


def channel_error(a, ref):
    """The largest error per channel over the image, divided by the channel's largest magnitude."""
    return np.abs(a.astype(np.float64) - ref).max(axis=0) / np.abs(ref).max(axis=0)


def foam_material(foam, **kw):
    """A material of roughness 0.3 whose foam threshold lies midway between the least and the most foam of the hit
    pixels (by the restatement), so that some of them foam and some do not wherever the foam varies at all."""
    lo, hi = (float(foam.min()), float(foam.max())) if len(foam) else (0.0, 0.0)
    return oh.material(roughness=0.3, foam_threshold=0.5 * (lo + hi) if hi > lo else 0.5, **kw)


def check_colour(ctx, tex, cam, slope, tile=0, split=False):
    """COLOR against the restatement: the status exactly, rgb by the yardstick.  split: some hit pixels must foam
    and some must not.  Returns the device image."""
    has_foam = tex.deriv is not None
    probe = shading_inputs(tex, cam, oh.material(lod_slope=slope), W, H, K, STEPS, REFINE)
    mat = foam_material(probe[5], lod_slope=slope)
    args = shading_inputs(tex, cam, mat, W, H, K, STEPS, REFINE)
    rec, foam = args[1], args[5]
    print(f"foam of the hit pixels: {foam.min()} .. {foam.max()}, threshold {mat[15]}, {(foam >= mat[15]).sum()} foam")
    if split:
        assert has_foam and (foam >= mat[15]).any() and (foam < mat[15]).any()
    want32 = colours(*args, mat, has_foam, f32)
    want64 = colours(*args, mat, has_foam, np.float64)
    got = ctx.camera(cam, W, H, oh.CAMERA_COLOR, mat, tile, K, STEPS, REFINE).reshape(W * H, 4)
    np.testing.assert_array_equal(got[:, 3], rec[:, 3])
    assert np.isfinite(got).all()
    yard = channel_error(want32[:, :3], want64[:, :3])
    err = channel_error(got[:, :3], want64[:, :3])
    print(f"lod_slope {slope}: restatement against float64 {yard}, device against float64 {err}, "
          f"factor {err / yard}")
    assert (yard > 0).all() and (err <= 4.0 * yard).all(), (err, yard)
    return got


@pytest.mark.parametrize("n,ncasc,flags", CONTEXTS)
def test_camera_matches_restatement(n, ncasc, flags):
    """HITS and RANGE bit for bit against the restatement and against ocean_raycast over the restatement's rays;
    COLOR's status exactly and its rgb within 4 x the fp32 restatement's own error against float64 (the two powf
    are the only operations that may differ).  The foam threshold splits the hit pixels wherever the scene has
    foam to split: not with cascade 0 alone, whose TURB.x stays above 1 at 64^2 (its foam, 1 - saturate, is 0 at
    every texel, which is asserted), and not on the DISPLACEMENT_ONLY context, which has none.  From below the
    surface every pixel is submerged."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = mip_textures(ctx, cas)
    bounds = ctx.surface_bounds()
    cam = pose_above(bounds)
    rays = camera_rays(cam, W, H)
    want = restate_camera(tex, cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE)
    check_shares(want[:, 3])
    hits = ctx.camera(cam, W, H, oh.CAMERA_HITS, None, 0, K, STEPS, REFINE)
    assert hits.shape == (H, W, 8)
    np.testing.assert_array_equal(hits.reshape(-1, 8), want)
    np.testing.assert_array_equal(hits.reshape(-1, 8), ctx.raycast(rays, iterations=K, steps=STEPS, refine=REFINE))
    rng = ctx.camera(cam, W, H, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE)
    assert rng.shape == (H, W)
    miss = want[:, 3] == oh.RAY_MISS
    np.testing.assert_array_equal(rng.ravel()[~miss], want[~miss, 0])
    np.testing.assert_array_equal(rng.ravel()[miss], f32(np.inf))
    np.testing.assert_array_equal(rng.ravel(), restate_camera(tex, cam, None, W, H, oh.CAMERA_RANGE, K, STEPS, REFINE))
    got = check_colour(ctx, tex, cam, 0.0, split=ncasc > 1 and not flags & oh.F_DISPLACEMENT_ONLY)
    if ncasc == 1:
        assert tex.turb[..., 0].min() >= 1.0
    if flags & oh.F_DISPLACEMENT_ONLY:
        np.testing.assert_array_equal(hits[..., 4:], np.tile(f32([0, 1, 0, 0]), (H, W, 1)))
    # the defaults of the binding: colour mode, K = 4, S = 64, B = 8
    mat = oh.material()
    np.testing.assert_array_equal(ctx.camera(cam, W, H, material=mat)[..., 3].ravel(),
                                  ctx.raycast(rays)[:, 3])
    # under water
    sub = pose_below(bounds)
    col = ctx.camera(sub, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
    np.testing.assert_array_equal(col.reshape(-1, 4), restate_camera(tex, sub, mat, W, H, oh.CAMERA_COLOR, K, STEPS, REFINE))
    np.testing.assert_array_equal(col.reshape(-1, 4), np.tile(np.r_[mat[0:3], f32(oh.RAY_SUBMERGED)], (W * H, 1)))
    np.testing.assert_array_equal(ctx.camera(sub, W, H, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE), f32(0))
    assert got.shape == (W * H, 4)
    ctx.close()


def test_camera_lod_path():
    """On the OCEAN_F_MIPS context a nonzero lod_slope changes the colours and matches the restatement's trilinear
    sample; on a context without mip chains it changes no bit."""
    cas = O.SCENE_CASCADES[:2]
    ctx = make_ctx(128, cas, oh.F_MIPS)
    tex = mip_textures(ctx, cas)
    cam = pose_above(ctx.surface_bounds())
    flat = check_colour(ctx, tex, cam, 0.0, split=True)
    slope = 0.01  # lod 0 at the eye, 4 at 400 m
    deep = check_colour(ctx, tex, cam, slope)
    hit = flat[:, 3] == oh.RAY_HIT
    changed = (flat[hit, :3] != deep[hit, :3]).any(axis=1).mean()
    print(f"{changed:.3f} of the hit pixels change colour with lod_slope = {slope}")
    assert changed > 0.9
    np.testing.assert_array_equal(flat[~hit], deep[~hit])
    ctx.close()
    plain = make_ctx(64, cas)
    cam = pose_above(plain.surface_bounds())
    a = plain.camera(cam, W, H, oh.CAMERA_COLOR, oh.material(lod_slope=0.0), 0, K, STEPS, REFINE)
    b = plain.camera(cam, W, H, oh.CAMERA_COLOR, oh.material(lod_slope=slope), 0, K, STEPS, REFINE)
    np.testing.assert_array_equal(a, b)
    plain.close()


def test_camera_air_skip_and_tile_mapping_change_no_bit():
    """OCEAN_RAY_BOUNDS=0 and =1, and the row-linear mapping of pixels to lanes (OCEAN_CAMERA_TILE=0), give
    identical images in all three modes, HITS being ocean_raycast's records of the restatement's rays; with the
    skip on two images in one frame launch the bounds kernels once."""
    n, cas = 64, O.SCENE_CASCADES[:3]
    on, _ = _ctx_with_env({"OCEAN_RAY_BOUNDS": "1"}, n, cas)
    off, _ = _ctx_with_env({"OCEAN_RAY_BOUNDS": "0"}, n, cas)
    lin, _ = _ctx_with_env({"OCEAN_CAMERA_TILE": "0"}, n, cas)
    for ctx in (on, off, lin):
        ctx.step(0.5)
        ctx.step(1.0)
    tex = Textures(on, cas)
    cam = pose_above(on.surface_bounds())
    rays = camera_rays(cam, W, H)
    want = restate_camera(tex, cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE)
    check_shares(want[:, 3])
    mat = oh.material(roughness=0.3)
    for ctx in (on, off, lin):
        hits = ctx.camera(cam, W, H, oh.CAMERA_HITS, None, 0, K, STEPS, REFINE).reshape(-1, 8)
        np.testing.assert_array_equal(hits, want)
        np.testing.assert_array_equal(hits, ctx.raycast(rays, iterations=K, steps=STEPS, refine=REFINE))
    for mode in (oh.CAMERA_RANGE, oh.CAMERA_COLOR):
        a = on.camera(cam, W, H, mode, mat, 0, K, STEPS, REFINE)
        np.testing.assert_array_equal(a, off.camera(cam, W, H, mode, mat, 0, K, STEPS, REFINE))
        np.testing.assert_array_equal(a, lin.camera(cam, W, H, mode, mat, 0, K, STEPS, REFINE))
    for ctx, launches in ((on, 3), (off, 2)):
        ctx.set_kernel_timing(True)
        ctx.step(1.5)
        ctx.kernel_stats(2)  # (reset: the frame itself may count kind-2 launches)
        ctx.camera(cam, W, H, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE)
        ctx.camera(cam, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
        ms, count = ctx.kernel_stats(2)
        assert count == launches and ms > 0, (count, launches)
        assert "k_camera" in ctx.kernel_name(2)
        ctx.set_kernel_timing(False)
    for ctx in (on, off, lin):
        ctx.close()


def test_camera_on_a_later_tile():
    """T = 2: the image of tile 1 is checked against tile 1's own textures, and tile 0's image differs."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, tiles=2)
    cam = pose_above(ctx.surface_bounds(1))
    want = restate_camera(Textures(ctx, cas, tile=1), cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE)
    check_shares(want[:, 3])
    got = ctx.camera(cam, W, H, oh.CAMERA_HITS, None, 1, K, STEPS, REFINE).reshape(-1, 8)
    np.testing.assert_array_equal(got, want)
    other = ctx.camera(cam, W, H, oh.CAMERA_HITS, None, 0, K, STEPS, REFINE).reshape(-1, 8)
    assert not np.array_equal(got, other)
    check_colour(ctx, Textures(ctx, cas, tile=1), cam, 0.0, tile=1)
    ctx.close()


def test_camera_forms_agree_and_async_snapshots_behind_later_steps():
    """The three forms agree bit for bit in every mode; the async request made after step t1, with two more steps
    queued right behind it, holds the image of t1 (a second context gives it), and the caller's camera and material,
    overwritten right after the call, are not read again.  An async result larger than a slot is refused."""
    import torch
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
    ref.step(times[0])
    cam = pose_above(ref.surface_bounds())
    mat = oh.material(roughness=0.3)
    cbuf, mbuf = cam.copy(), mat.copy()
    ctx.step(times[0])
    rb = ctx.camera_async(cbuf, W, H, oh.CAMERA_COLOR, mbuf, 0, K, STEPS, REFINE)
    cbuf[:], mbuf[:] = 1.0e9, 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    rb.release()
    want = ref.camera(cam, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
    check_shares(want[..., 3].ravel())
    np.testing.assert_array_equal(got, want)
    later = ctx.camera(cam, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)  # the blocking form now: frame t3
    assert not np.array_equal(got, later)
    dev = torch.device("cuda", ctx.device)
    for mode, per in ((oh.CAMERA_HITS, 8), (oh.CAMERA_RANGE, 1), (oh.CAMERA_COLOR, 4)):
        m = mat if mode == oh.CAMERA_COLOR else None
        block = ctx.camera(cam, W, H, mode, m, 0, K, STEPS, REFINE)
        slot = oh.PinnedBuffer(W * H * per * 4)
        rb = ctx.camera_async(cam, W, H, mode, m, 0, K, STEPS, REFINE, buf=slot)
        np.testing.assert_array_equal(rb.data, block)
        rb.release()
        slot.release()
        o = torch.full((W * H * per + 4,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.camera_device(o.data_ptr(), cam, W, H, mode, m, 0, K, STEPS, REFINE)
        ctx.synchronize()
        np.testing.assert_array_equal(o[:W * H * per].cpu().numpy().reshape(block.shape), block)
        np.testing.assert_array_equal(o[W * H * per:].cpu().numpy(), f32(-1))  # nothing past the image
    # 320 x 320 records of 32 B = 3,276,800 B > a slot of max(256 * 256 * 16, 65536 * 40) = 2,621,440 B
    with pytest.raises(oh.OceanError) as e:
        ctx.camera_async(cam, 320, 320, oh.CAMERA_HITS, None, 0, K, 1, 0)
    assert e.value.code == oh.E_INVALID_ARG and "slot" in str(e.value)
    assert ctx.camera(cam, 320, 320, oh.CAMERA_RANGE, None, 0, 0, 1, 0).shape == (320, 320)  # the blocking form serves it
    ctx.close()
    ref.close()


def test_camera_errors_on_a_context():
    """OCEAN_E_STATE before ocean_init_spectrum, a tile out of range, a misaligned device `out`, and
    OCEAN_E_UNSUPPORTED on a column-parity context; *req is NULL after each."""
    import torch
    cam = oh.look_at_camera((0, 20, 0), (30, 10, 40), (0, 1, 0), 0.9, W, H, 0.0, 200.0)
    mat = oh.material()
    ctx = oh.OceanContext(64, 2, 1)
    for call in (ctx.camera, ctx.camera_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, material=mat)
        assert e.value.code == oh.E_STATE and "ocean_init_spectrum" in str(e.value)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    for tile in (1, -1):
        for call in (ctx.camera, ctx.camera_async):
            with pytest.raises(oh.OceanError) as e:
                call(cam, W, H, material=mat, tile=tile)
            assert e.value.code == oh.E_INVALID_ARG and "tile" in str(e.value)
    L, h, vp = ctx.lib, ctx._h, ctypes.c_void_p
    o = torch.zeros(W * H * 4 + 4, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    assert L.ocean_camera_device(h, 0, oh.CAMERA_COLOR, K, STEPS, REFINE, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H,
                                 vp(o.data_ptr() + 4), W * H * 16) == oh.E_INVALID_ARG
    assert b"aligned" in L.ocean_last_error()
    req = ctypes.c_void_p(0x1234)
    out = np.zeros(W * H * 4, f32)
    assert L.ocean_camera_async(h, 0, oh.CAMERA_COLOR, K, STEPS, REFINE, vp(cam.ctypes.data), None, W, H,
                                vp(out.ctypes.data), W * H * 16, ctypes.byref(req)) == oh.E_INVALID_ARG
    assert req.value is None and b"material" in L.ocean_last_error()
    ctx.synchronize()
    assert not o.cpu().numpy().any()
    ctx.close()
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    for call in (par.camera, par.camera_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, material=mat)
        assert e.value.code == oh.E_UNSUPPORTED
    par.close()


def test_water_body_camera_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    wb.Update(0.5)
    eye, target = (3.0, 12.0, -4.0), (40.0, 4.0, 50.0)
    cam = oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 1.0, W, H, 0.0, 2000.0)
    img = wb.Camera(eye, target, W, H)
    assert img.shape == (H, W, 4)
    np.testing.assert_array_equal(img, wb.ctx.camera(cam, W, H, oh.CAMERA_COLOR, oh.material()))
    rng = wb.Camera(eye, target, W, H, mode=oh.CAMERA_RANGE, max_distance=300.0, steps=32)
    cam = oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 1.0, W, H, 0.0, 300.0)
    np.testing.assert_array_equal(rng, wb.ctx.camera(cam, W, H, oh.CAMERA_RANGE, steps=32))
    assert np.isinf(rng).any() and np.isfinite(rng).any()
    wb.OnDisable()
