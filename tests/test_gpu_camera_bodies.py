"""GPU tests of the camera views that see the bodies (ocean_camera_bodies / _device / _async, csrc/view.hip,
k_camera_bodies) against restate_camera_bodies (tests/test_camera_bodies_abi.py: numpy fp32, every body tried for every
pixel) applied to the context's own read-back textures.  The ray records and the range image are compared bit for
bit, the body's index and normal included; the colours by the camera's yardstick (tests/test_gpu_camera.py): the
device's error against a float64 evaluation is at most 4 x the fp32 restatement's own, per channel.

The image is 45 x 37 (partial tiles on both edges), K = 2, S = 32, B = 6, the camera test_gpu_camera.py's pose_above.
scatter_boxes puts rotated, non-uniformly scaled boxes over the viewed patch at heights around the water level, their
size growing with the distance so that each covers a few pixels; its constants were chosen on the CPU with the
restatement over the oracle's textures of the same scenes, and every test asserts the shares it needs on the
restatement alone."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_camera_bodies_abi import restate_camera_bodies
from test_gpu_camera import H, K, REFINE, STEPS, W, channel_error, mip_textures, pose_above
from test_gpu_parity import _ctx_with_env
from test_gpu_query import Textures, make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
CONTEXTS = [(64, 1, 0), (64, 4, 0), (128, 2, oh.F_MIPS)]
BOX = f32([-0.5, -0.25, -0.5, 0.5, 0.75, 0.5])  # off centre: the body's origin is a quarter up from the keel
PAINT = f32([0.85, 0.35, 0.15, 0.6])
SKY = oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT
MODES = ((oh.CAMERA_HITS, 8), (oh.CAMERA_RANGE, 1), (oh.CAMERA_COLOR, 4))


def scatter_boxes(cam, count, seed=7, stride=10):
    """`count` records float32[count][stride]: boxes in the camera's horizontal field of view, 12 to 350 m from the
    eye (log-uniform, so that near and far are both there), their origins within a few metres of the mean water level,
    each side 3 to 9 % of the distance, any orientation (unit quaternions, normalised in float64 and rounded once).
    One box alone stands 30 m ahead.  The floats behind the tenth are junk that the entry must not read."""
    rng = np.random.default_rng(seed)
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (W - 1) / 2 + c[9:12] * (H - 1) / 2
    heading = np.arctan2(ahead[0], ahead[2])
    half = np.arctan(np.linalg.norm(c[6:9]) * W / 2)
    rec = np.random.default_rng(seed + 1).uniform(-1e3, 1e3, (count, stride))  # (the boxes do not depend on the stride)
    ang = heading + half * rng.uniform(-0.95, 0.95, count)
    r = 12.0 * (350.0 / 12.0) ** rng.uniform(0, 1, count)
    if count == 1:
        ang, r = np.float64([heading + 0.05]), np.float64([30.0])
    rec[:, 0], rec[:, 2] = c[0] + r * np.sin(ang), c[2] + r * np.cos(ang)
    rec[:, 1] = rng.uniform(-2.0, 2.5, count)
    q = rng.normal(size=(count, 4))
    rec[:, 3:7] = q / np.linalg.norm(q, axis=1)[:, None]
    rec[:, 7:10] = r[:, None] * rng.uniform(0.03, 0.09, (count, 3))
    if count == 1:
        rec[:, 7:10] = (7.0, 4.0, 9.0)
    return rec.astype(f32)


def shares(info):
    """What the restatement's image holds: the shares of body, water-hit and miss pixels, the pixels where a body is
    met but the water wins, and those where both are met and the body wins."""
    rec, b, body = info["rec"], info["b"], info["body"]
    return dict(body=body.mean(), hit=(~body & (rec[:, 3] == oh.RAY_HIT)).mean(),
                miss=(~body & (rec[:, 3] == oh.RAY_MISS)).mean(),
                water_wins=int(((b >= 0) & ~body).sum()), body_wins=int((body & (rec[:, 3] == oh.RAY_HIT)).sum()))


def check_shares(info):
    s = shares(info)
    print(s)
    assert s["body"] >= 0.1 and s["hit"] >= 0.2 and s["miss"] >= 0.1 and s["water_wins"] >= 20 and s["body_wins"] >= 20, s


def check_colour(ctx, tex, cam, mat, bodies, mode=oh.CAMERA_COLOR, sky=None, tile=0):
    want32, info = restate_camera_bodies(tex, cam, mat, W, H, mode, K, STEPS, REFINE, BOX, PAINT, bodies, f32, sky)
    want64, _ = restate_camera_bodies(tex, cam, mat, W, H, mode, K, STEPS, REFINE, BOX, PAINT, bodies, np.float64, sky)
    got = ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, mode, mat, tile, K, STEPS, REFINE).reshape(W * H, 4)
    np.testing.assert_array_equal(got[:, 3], want32[:, 3])
    assert np.isfinite(got).all()
    yard = channel_error(want32[:, :3], want64[:, :3])
    err = channel_error(got[:, :3], want64[:, :3])
    print(f"mode {mode}: restatement against float64 {yard}, device against float64 {err}, factor {err / yard}")
    assert (yard > 0).all() and (err <= 4.0 * yard).all(), (err, yard)
    body = info["body"]  # the bodies' own pixels by the same yardstick (their formula has no powf: the error is small)
    if body.any():
        yard = channel_error(want32[body, :3], want64[body, :3])
        err = channel_error(got[body, :3], want64[body, :3])
        print(f"  body pixels: restatement {yard}, device {err}")
        assert (err <= 4.0 * yard).all(), (err, yard)
    return got


def test_empty_list_is_ocean_camera_bit_for_bit():
    """count = 0, with `bodies` NULL or an empty array: all four modes equal ocean_camera's image."""
    cas = O.SCENE_CASCADES[:2]
    ctx = make_ctx(64, cas)
    cam = pose_above(ctx.surface_bounds())
    ctx.atmosphere()
    sun = (0.3, 0.25, 0.9)
    ctx.sky_update(sun)
    mat = oh.material(roughness=0.3, light_direction=sun, light_color=ctx.sun_color(sun))
    for mode in (oh.CAMERA_HITS, oh.CAMERA_RANGE, oh.CAMERA_COLOR, SKY):
        want = ctx.camera(cam, W, H, mode, mat, 0, K, STEPS, REFINE)
        for bodies in (None, np.zeros((0, 10), f32)):
            got = ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE)
            np.testing.assert_array_equal(got, want)
    assert (want[..., 3] == oh.RAY_HIT).mean() >= 0.2 and (want[..., 3] == oh.RAY_MISS).mean() >= 0.1
    ctx.close()


@pytest.mark.parametrize("n,ncasc,flags", CONTEXTS)
def test_camera_bodies_match_restatement(n, ncasc, flags):
    """One box, and 300: more than a chunk of 256, so the chunk loop runs twice, the second chunk is partial and the
    survivors of the first come from all four waves.  HITS and RANGE bit for bit, COLOR's status exactly and its
    rgb by the yardstick.  The records are 13 floats apart with junk behind the tenth."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = mip_textures(ctx, cas)
    cam = pose_above(ctx.surface_bounds())
    mat = oh.material(roughness=0.3, lod_slope=0.004)
    for count in (1, 300):
        bodies = scatter_boxes(cam, count, stride=13)
        want, info = restate_camera_bodies(tex, cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE, BOX, None, bodies)
        if count == 300:
            check_shares(info)
            assert len(set(info["b"][info["body"]])) >= 40 and info["b"].max() >= 256  # many bodies, of both chunks
        else:
            assert info["body"].sum() >= 20
        hits = ctx.camera_bodies(cam, W, H, bodies, BOX, None, oh.CAMERA_HITS, None, 0, K, STEPS, REFINE)
        assert hits.shape == (H, W, 8)
        np.testing.assert_array_equal(hits.reshape(-1, 8), want)
        rng = ctx.camera_bodies(cam, W, H, bodies, BOX, None, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE)
        want_rng, _ = restate_camera_bodies(tex, cam, None, W, H, oh.CAMERA_RANGE, K, STEPS, REFINE, BOX, None, bodies)
        np.testing.assert_array_equal(rng.ravel(), want_rng)
        check_colour(ctx, tex, cam, mat, bodies)
    ctx.close()


def test_sky_lut_mode_paints_the_bodies_under_the_table():
    """COLOR | SKY_LUT: amb is SKY(nw) of the context's own sky-view table; the camera's state rules hold (the table
    absent or stale: OCEAN_E_STATE, after the argument checks)."""
    cas = O.SCENE_CASCADES[:1]
    ctx = make_ctx(64, cas)
    tex = Textures(ctx, cas)
    cam = pose_above(ctx.surface_bounds())
    bodies = scatter_boxes(cam, 300)
    sun = (0.3, 0.25, 0.9)
    plain = oh.material(roughness=0.3)
    for call in (ctx.camera_bodies, ctx.camera_bodies_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, bodies, BOX, PAINT, SKY, plain, 0, K, STEPS, REFINE)
        assert e.value.code == oh.E_STATE
    ctx.atmosphere()
    with pytest.raises(oh.OceanError) as e:
        ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, SKY, plain, 0, K, STEPS, REFINE)
    assert e.value.code == oh.E_STATE and "ocean_sky_update" in str(e.value)
    with pytest.raises(oh.OceanError) as e:
        ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, SKY, plain, 0, K, 0, REFINE)
    assert e.value.code == oh.E_INVALID_ARG and "steps" in str(e.value)
    ctx.sky_update(sun)
    mat = oh.material(roughness=0.3, light_direction=sun, light_color=ctx.sun_color(sun))
    S = ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    got = check_colour(ctx, tex, cam, mat, bodies, SKY, (S, oh.atmosphere_params()[26]))
    two = ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE).reshape(-1, 4)
    body = got[:, 3] == oh.RAY_BODY
    assert body.mean() >= 0.1 and (got[body, :3] != two[body, :3]).any(axis=1).mean() > 0.9
    ctx.close()


def test_time_only_switches_change_no_bit():
    """OCEAN_CAMERA_CULL=0, OCEAN_RAY_BOUNDS=0 and the defaults give one image in every mode: the cull and the early
    stop of the march decide which tests and samples are made, never a bit.  Besides the 300 boxes the scene has a box
    wholly under the lowest trough in the middle of the view, which every ray meets behind the water, and a small box
    in the air close to the eye, in front of water that the full march hits."""
    n, cas = 64, O.SCENE_CASCADES[:3]
    ctxs = [_ctx_with_env(env, n, cas)[0] for env in ({"OCEAN_CAMERA_CULL": "0"}, {"OCEAN_RAY_BOUNDS": "0"}, {})]
    for ctx in ctxs:
        ctx.step(0.5)
        ctx.step(1.0)
    ref = ctxs[2]
    tex = Textures(ref, cas)
    bounds = ref.surface_bounds()
    cam = pose_above(bounds)
    c = cam.astype(np.float64)
    ahead = c[3:6] + c[6:9] * (W - 1) / 2 + c[9:12] * (H - 1) / 2
    low = float(bounds[:, 1].astype(np.float64).sum())
    sunk = np.r_[c[0:3] + 35.0 * ahead, 0, 0, 0, 1, 30, 2, 30]
    sunk[1] = low - 4.0  # BOX reaches 0.75 * 2 above the origin: still 2.5 m under every trough
    air = np.r_[c[0:3] + 8.0 * ahead + [0.0, -0.4, 0.0], 0, 0.6, 0, 0.8, 1.8, 1.1, 0.9]
    bodies = np.concatenate([scatter_boxes(cam, 300), f32([sunk, air])])
    want, info = restate_camera_bodies(tex, cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE, BOX, None, bodies)
    check_shares(info)
    rec, b, body = info["rec"], info["b"], info["body"]
    under = b == 300
    assert under.sum() >= 20 and not body[under].any() and (rec[under, 3] == oh.RAY_HIT).all()
    front = b == 301
    assert front.sum() >= 20 and body[front].all() and (rec[front, 3] == oh.RAY_HIT).sum() >= 20
    mat = oh.material(roughness=0.3)
    for mode, per in MODES:
        imgs = [ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE) for ctx in ctxs]
        np.testing.assert_array_equal(imgs[0], imgs[2])
        np.testing.assert_array_equal(imgs[1], imgs[2])
        if mode == oh.CAMERA_HITS:
            np.testing.assert_array_equal(imgs[2].reshape(-1, 8), want)
    ref.set_kernel_timing(True)
    ref.kernel_stats(2)
    ref.camera_bodies(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE)
    ms, launches = ref.kernel_stats(2)
    assert launches == 1 and ms > 0 and "k_camera_bodies" in ref.kernel_name(2)
    for ctx in ctxs:
        ctx.close()


def test_device_form_over_the_result_of_body_step_device():
    """ocean_camera_bodies_device over the `out` of ocean_body_step_device, stride 32, where it lies, equals
    ocean_camera_bodies over the first ten floats of the landed records, stride 10."""
    import torch
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, oh.F_VELOCITY)
    cam = pose_above(ctx.surface_bounds())
    count = 300
    poses = scatter_boxes(cam, count)
    poses[:, 1] += 1.0
    hull = oh.OceanContext.box_hull(2, 2)
    state = oh.OceanContext.body_state(poses)
    props = np.tile(f32([0.01, 0.02, 0.02, 0.02]), (count, 1))
    step = oh.step_params(1.0 / 120.0)
    dev = torch.device("cuda", ctx.device)
    d_hull, d_props, d_state = (torch.from_numpy(a).to(dev) for a in (hull, props, state))
    d_out = torch.zeros((count, 32), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.body_step_device(d_hull.data_ptr(), len(hull), d_props.data_ptr(), d_state.data_ptr(), count, d_out.data_ptr(), step,
                         substeps=8)
    mat = oh.material(roughness=0.3)
    imgs = {}
    for mode, per in MODES:
        o = torch.full((W * H * per + 4,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.camera_bodies_device(o.data_ptr(), cam, W, H, d_out.data_ptr(), count, 32, BOX, PAINT, mode, mat, 0, K, STEPS,
                                 REFINE)
        ctx.synchronize()
        imgs[mode] = o[:W * H * per].cpu().numpy()
        np.testing.assert_array_equal(o[W * H * per:].cpu().numpy(), f32(-1))  # nothing past the image
    landed = d_out.cpu().numpy()
    assert not np.array_equal(landed[:, :10], poses)  # the bodies moved
    for mode, per in MODES:
        want = ctx.camera_bodies(cam, W, H, np.ascontiguousarray(landed[:, :10]), BOX, PAINT, mode, mat, 0, K, STEPS, REFINE)
        np.testing.assert_array_equal(imgs[mode], want.ravel())
        np.testing.assert_array_equal(ctx.camera_bodies(cam, W, H, landed, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE), want)
    assert (imgs[oh.CAMERA_HITS].reshape(-1, 8)[:, 3] == oh.RAY_BODY).mean() >= 0.1
    ctx.close()


def test_camera_bodies_on_a_later_tile():
    """T = 2: tile 1's image is checked against tile 1's own textures, and tile 0's differs."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, tiles=2)
    cam = pose_above(ctx.surface_bounds(1))
    bodies = scatter_boxes(cam, 300)
    tex = Textures(ctx, cas, tile=1)
    want, info = restate_camera_bodies(tex, cam, None, W, H, oh.CAMERA_HITS, K, STEPS, REFINE, BOX, None, bodies)
    check_shares(info)
    got = ctx.camera_bodies(cam, W, H, bodies, BOX, None, oh.CAMERA_HITS, None, 1, K, STEPS, REFINE).reshape(-1, 8)
    np.testing.assert_array_equal(got, want)
    other = ctx.camera_bodies(cam, W, H, bodies, BOX, None, oh.CAMERA_HITS, None, 0, K, STEPS, REFINE).reshape(-1, 8)
    assert not np.array_equal(got, other)
    check_colour(ctx, tex, cam, oh.material(roughness=0.3), bodies, tile=1)
    ctx.close()


def test_forms_agree_and_async_snapshots_behind_later_steps():
    """The three forms agree bit for bit in every mode; the async request made after step t1, with two more steps
    queued right behind it, holds the image of t1, and the caller's arrays, overwritten right after the call, are not
    read again.  An async result larger than a slot is refused; the blocking form serves it."""
    import torch
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
    ref.step(times[0])
    cam = pose_above(ref.surface_bounds())
    mat = oh.material(roughness=0.3)
    bodies = scatter_boxes(cam, 300, stride=32)
    cbuf, mbuf, bbuf, xbuf, pbuf = cam.copy(), mat.copy(), bodies.copy(), BOX.copy(), PAINT.copy()
    ctx.step(times[0])
    rb = ctx.camera_bodies_async(cbuf, W, H, bbuf, xbuf, pbuf, oh.CAMERA_COLOR, mbuf, 0, K, STEPS, REFINE)
    for a in (cbuf, mbuf, bbuf, xbuf, pbuf):
        a[:] = 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    rb.release()
    want = ref.camera_bodies(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
    status = want[..., 3].ravel()
    assert (status == oh.RAY_BODY).mean() >= 0.1 and (status == oh.RAY_HIT).mean() >= 0.2
    np.testing.assert_array_equal(got, want)
    later = ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)  # frame t3
    assert not np.array_equal(got, later)
    dev = torch.device("cuda", ctx.device)
    d_bodies = torch.from_numpy(bodies).to(dev)
    for mode, per in MODES:
        block = ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE)
        slot = oh.PinnedBuffer(W * H * per * 4)
        rb = ctx.camera_bodies_async(cam, W, H, bodies, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE, buf=slot)
        np.testing.assert_array_equal(rb.data, block)
        rb.release()
        slot.release()
        o = torch.full((W * H * per + 4,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.camera_bodies_device(o.data_ptr(), cam, W, H, d_bodies.data_ptr(), len(bodies), 32, BOX, PAINT, mode, mat, 0, K,
                                 STEPS, REFINE)
        ctx.synchronize()
        np.testing.assert_array_equal(o[:W * H * per].cpu().numpy().reshape(block.shape), block)
        np.testing.assert_array_equal(o[W * H * per:].cpu().numpy(), f32(-1))
    # an empty list in the async form is a request like any other
    rb = ctx.camera_bodies_async(cam, W, H, None, BOX, None, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE)
    np.testing.assert_array_equal(rb.data, ctx.camera(cam, W, H, oh.CAMERA_RANGE, None, 0, K, STEPS, REFINE))
    rb.release()
    # 320 x 320 records of 32 B = 3,276,800 B > a slot of max(256 * 256 * 16, 65536 * 40) = 2,621,440 B
    with pytest.raises(oh.OceanError) as e:
        ctx.camera_bodies_async(cam, 320, 320, bodies, BOX, None, oh.CAMERA_HITS, None, 0, K, 1, 0)
    assert e.value.code == oh.E_INVALID_ARG and "slot" in str(e.value) and "ocean_camera_bodies_async" in str(e.value)
    assert ctx.camera_bodies(cam, 320, 320, bodies, BOX, None, oh.CAMERA_RANGE, None, 0, 0, 1, 0).shape == (320, 320)
    # a misaligned device `bodies`, and the state rule before ocean_init_spectrum
    L, vp = ctx.lib, ctypes.c_void_p
    o = torch.zeros(W * H + 4, dtype=torch.float32, device=dev)
    assert L.ocean_camera_bodies_device(ctx._h, 0, oh.CAMERA_RANGE, K, STEPS, REFINE, vp(cam.ctypes.data), None, W, H,
                                        vp(BOX.ctypes.data), None, vp(d_bodies.data_ptr() + 2), 32, 4, vp(o.data_ptr()),
                                        W * H * 4) == oh.E_INVALID_ARG
    assert b"aligned" in L.ocean_last_error()
    ctx.close()
    ref.close()
    bare = oh.OceanContext(64, 2, 1)
    for call in (bare.camera_bodies, bare.camera_bodies_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_COLOR, mat)
        assert e.value.code == oh.E_STATE and "ocean_init_spectrum" in str(e.value)
    bare.close()


def test_water_body_camera_bodies_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    wb.Update(0.5)
    eye, target = (3.0, 12.0, -4.0), (40.0, 4.0, 50.0)
    cam = oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 1.0, W, H, 0.0, 2000.0)
    bodies = scatter_boxes(cam, 64)
    img = wb.camera_bodies(eye, target, W, H, bodies, BOX, PAINT)
    assert img.shape == (H, W, 4) and (img[..., 3] == oh.RAY_BODY).any()
    np.testing.assert_array_equal(img, wb.ctx.camera_bodies(cam, W, H, bodies, BOX, PAINT, oh.CAMERA_COLOR, oh.material()))
    wb.OnDisable()
