"""GPU tests of the camera views in which the water sees the bodies (ocean_camera_scene / _device / _async,
csrc/view.hip, k_camera_scene) against restate_camera_scene (tests/test_camera_scene_abi.py: numpy, every body tried
for every primary and secondary ray, every decision in fp32) applied to the context's own read-back textures.  The
LINKS image, which holds every discrete decision, is compared bit for bit; the colours by the camera's yardstick
(tests/test_gpu_camera.py): the device's error against a float64 shading is at most 4 x the fp32 restatement's own,
per channel, over all pixels and over the linked water pixels alone.

The image is 45 x 37 (partial tiles on both edges), K = 2, S = 32, B = 6, the camera test_gpu_camera.py's pose_above.
The scene is test_camera_scene_abi.scene_boxes: 300 scattered boxes, a sunk one, a near one and four tall ones standing
in the water under a low sun.  Its constants were chosen on the CPU over the oracle's textures, and every test asserts
the shares it needs on the restatement alone."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_camera_scene_abi import (BOX, OPTICS, PAINT, SKY, SUN, check_link_shares, link_shares, restate_camera_scene,
                                   scene_boxes)
from test_gpu_camera import H, K, REFINE, STEPS, W, channel_error, mip_textures, pose_above
from test_gpu_parity import _ctx_with_env
from test_gpu_query import Textures, make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
CONTEXTS = [(64, 1, 0), (64, 4, 0), (128, 2, oh.F_MIPS)]
LINKS = oh.CAMERA_LINKS


def sun_material(**kw):
    return oh.material(roughness=0.3, light_direction=SUN, **kw)


def scene(ctx, tile=0, stride=10):
    bounds = ctx.surface_bounds(tile)
    cam = pose_above(bounds)
    return cam, scene_boxes(cam, bounds, W, H, stride)


def shoot(ctx, cam, bodies, mode, mat, optics=OPTICS, tile=0, paint=PAINT):
    return ctx.camera_scene(cam, W, H, bodies, BOX, paint, optics, mode, mat, tile, K, STEPS, REFINE)


@pytest.mark.parametrize("n,ncasc,flags", CONTEXTS)
def test_links_match_restatement(n, ncasc, flags):
    """The LINKS image bit for bit: one box, the 302 boxes of the camera-bodies tests, and the whole scene, whose
    linked bodies come from both chunks of 256.  The records are 13 floats apart with junk behind the tenth."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = mip_textures(ctx, cas)
    cam, bodies = scene(ctx, stride=13)
    mat = sun_material(lod_slope=0.004)
    for count in (1, 302, len(bodies)):
        want, info = restate_camera_scene(tex, cam, mat, W, H, LINKS, K, STEPS, REFINE, BOX, None, OPTICS, bodies[:count])
        if count == len(bodies):
            check_link_shares(info)
        elif count == 302:
            s = link_shares(info)
            assert min(s["shadowed"], s["through"], s["mirrored"], s["free"]) >= 20 and s["top"] >= 256, s
        got = shoot(ctx, cam, bodies[:count], LINKS, mat, paint=None)
        assert got.shape == (H, W, 4)
        np.testing.assert_array_equal(got.reshape(-1, 4), want)
    ctx.close()


def check_colour(ctx, tex, cam, mat, bodies, mode=oh.CAMERA_COLOR, sky=None, tile=0):
    want32, info = restate_camera_scene(tex, cam, mat, W, H, mode, K, STEPS, REFINE, BOX, PAINT, OPTICS, bodies, f32, sky)
    want64, _ = restate_camera_scene(tex, cam, mat, W, H, mode, K, STEPS, REFINE, BOX, PAINT, OPTICS, bodies, np.float64, sky)
    check_link_shares(info)
    got = shoot(ctx, cam, bodies, mode, mat, tile=tile).reshape(W * H, 4)
    np.testing.assert_array_equal(got[:, 3], want32[:, 3])
    assert np.isfinite(got).all()
    linked = (info["sf"] == 0) | (info["b1t"] >= 0) | (info["b2"] >= 0)
    for name, rows in (("all pixels", slice(None)), ("linked water pixels", linked), ("through-water pixels", info["b1t"] >= 0)):
        yard = channel_error(want32[rows, :3], want64[rows, :3])
        err = channel_error(got[rows, :3], want64[rows, :3])
        print(f"mode {mode}, {name}: restatement against float64 {yard}, device against float64 {err}, factor {err / yard}")
        assert (yard > 0).all() and (err <= 4.0 * yard).all(), (name, err, yard)
    return got, info


@pytest.mark.parametrize("n,ncasc,flags", CONTEXTS)
def test_colour_matches_restatement(n, ncasc, flags):
    """COLOR: the status exactly, rgb by the yardstick, over all pixels and over the linked water pixels (exp2f is
    on the through-water pixels only, so they are measured alone as well)."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    tex = mip_textures(ctx, cas)
    cam, bodies = scene(ctx)
    check_colour(ctx, tex, cam, sun_material(lod_slope=0.004), bodies)
    ctx.close()


def test_sky_lut_mode():
    """COLOR | SKY_LUT: the reflection that meets no body and the bodies' ambient light read the context's own sky-view
    table; the camera's state rules hold (the table absent or stale: OCEAN_E_STATE, after the argument checks)."""
    cas = O.SCENE_CASCADES[:1]
    ctx = make_ctx(64, cas)
    tex = Textures(ctx, cas)
    cam, bodies = scene(ctx)
    plain = sun_material()
    for call in (ctx.camera_scene, ctx.camera_scene_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, bodies, BOX, PAINT, OPTICS, SKY, plain, 0, K, STEPS, REFINE)
        assert e.value.code == oh.E_STATE
    ctx.atmosphere()
    with pytest.raises(oh.OceanError) as e:
        shoot(ctx, cam, bodies, SKY, plain)
    assert e.value.code == oh.E_STATE and "ocean_sky_update" in str(e.value)
    with pytest.raises(oh.OceanError) as e:
        shoot(ctx, cam, bodies, SKY, plain, optics=oh.optics(reach=-1.0))
    assert e.value.code == oh.E_INVALID_ARG and "reach" in str(e.value)
    ctx.sky_update(SUN)
    mat = sun_material(light_color=ctx.sun_color(SUN))
    S = ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    got, info = check_colour(ctx, tex, cam, mat, bodies, SKY, (S, oh.atmosphere_params()[26]))
    two = shoot(ctx, cam, bodies, oh.CAMERA_COLOR, mat).reshape(-1, 4)
    wp = info["wp"]
    assert (got[wp, :3] != two[wp, :3]).any(axis=1).mean() > 0.9
    ctx.close()


def test_unlinked_pixels_are_ocean_camera_bodies_bit_for_bit():
    """count == 0 (NULL and empty) is ocean_camera_bodies' COLOR image in both sky modes; on the 302-box scene every
    pixel whose LINKS record is (1, -1, -1, .) is ocean_camera_bodies' pixel."""
    cas = O.SCENE_CASCADES[:2]
    ctx = make_ctx(64, cas)
    cam, bodies = scene(ctx)
    ctx.atmosphere()
    ctx.sky_update(SUN)
    mat = sun_material(light_color=ctx.sun_color(SUN))
    for mode in (oh.CAMERA_COLOR, SKY):
        want = ctx.camera_bodies(cam, W, H, None, BOX, PAINT, mode, mat, 0, K, STEPS, REFINE)
        for none in (None, np.zeros((0, 10), f32)):
            np.testing.assert_array_equal(shoot(ctx, cam, none, mode, mat), want)
        assert (want[..., 3] == oh.RAY_HIT).mean() >= 0.2 and (want[..., 3] == oh.RAY_MISS).mean() >= 0.1
    want, info = restate_camera_scene(Textures(ctx, cas), cam, mat, W, H, LINKS, K, STEPS, REFINE, BOX, None, OPTICS,
                                      bodies[:302])
    s = link_shares(info)
    assert min(s["shadowed"], s["through"], s["mirrored"], s["free"]) >= 20 and info["body"].sum() >= 100, s
    links = shoot(ctx, cam, bodies[:302], LINKS, mat).reshape(-1, 4)
    np.testing.assert_array_equal(links, want)
    free = (links[:, 0] == 1) & (links[:, 1] == -1) & (links[:, 2] == -1)
    water = links[:, 3] == oh.RAY_HIT
    for mode in (oh.CAMERA_COLOR, SKY):
        got = shoot(ctx, cam, bodies[:302], mode, mat).reshape(-1, 4)
        want = ctx.camera_bodies(cam, W, H, bodies[:302], BOX, PAINT, mode, mat, 0, K, STEPS, REFINE).reshape(-1, 4)
        np.testing.assert_array_equal(got[free], want[free])
        np.testing.assert_array_equal(got[~water], want[~water])  # body, MISS and SUBMERGED pixels too
        assert (got[~free & water, :3] != want[~free & water, :3]).any(axis=1).mean() > 0.9
    ctx.close()


def test_time_only_switches_change_no_bit():
    """OCEAN_CAMERA_CULL=0, OCEAN_RAY_BOUNDS=0 and the defaults give one LINKS image and one COLOR image: both culls and
    the early stop of the march decide which tests and samples are made, never a bit."""
    n, cas = 64, O.SCENE_CASCADES[:3]
    ctxs = [_ctx_with_env(env, n, cas)[0] for env in ({"OCEAN_CAMERA_CULL": "0"}, {"OCEAN_RAY_BOUNDS": "0"}, {})]
    for ctx in ctxs:
        ctx.step(0.5)
        ctx.step(1.0)
    ref = ctxs[2]
    tex = Textures(ref, cas)
    cam, bodies = scene(ref)
    mat = sun_material()
    want, info = restate_camera_scene(tex, cam, mat, W, H, LINKS, K, STEPS, REFINE, BOX, None, OPTICS, bodies)
    check_link_shares(info)
    for mode in (LINKS, oh.CAMERA_COLOR):
        imgs = [shoot(ctx, cam, bodies, mode, mat) for ctx in ctxs]
        np.testing.assert_array_equal(imgs[0], imgs[2])
        np.testing.assert_array_equal(imgs[1], imgs[2])
        if mode == LINKS:
            np.testing.assert_array_equal(imgs[2].reshape(-1, 4), want)
    ref.set_kernel_timing(True)
    ref.kernel_stats(2)
    shoot(ref, cam, bodies, LINKS, mat)
    ms, launches = ref.kernel_stats(2)
    assert launches == 1 and ms > 0 and "k_camera_scene" in ref.kernel_name(2)
    for ctx in ctxs:
        ctx.close()


def test_large_image_with_a_short_reach_equals_the_cull_off_image():
    """1024 x 1024 pixels, reach = 5 m: 4,096 tiles, most of which drop most bodies in the second cull, many with no
    water pixel at all.  No restatement: the image equals the one with every body a survivor.  One launch each."""
    n, cas, side = 64, O.SCENE_CASCADES[:2], 1024
    off, on = (_ctx_with_env(env, n, cas)[0] for env in ({"OCEAN_CAMERA_CULL": "0"}, {}))
    for ctx in (off, on):
        ctx.step(0.5)
        ctx.step(1.0)
    bounds = on.surface_bounds()
    small = pose_above(bounds)
    eye, ahead = small[0:3].astype(np.float64), np.float64([0.6, 0.0, 0.8])
    target = eye + 100.0 * ahead + np.float64([0.0, -100.0 * np.tan(np.radians(8.0)), 0.0])
    cam = oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 0.9, side, side, 0.0, 400.0)
    bodies = scene_boxes(small, bounds, W, H)
    near = oh.optics(shadow_color=(0.02, 0.03, 0.08), shadow_intensity=0.6, fog_density=0.15, reach=5.0)
    mat = sun_material()
    imgs = [ctx.camera_scene(cam, side, side, bodies, BOX, PAINT, near, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
            for ctx in (off, on)]
    np.testing.assert_array_equal(imgs[0], imgs[1])
    status = imgs[1][..., 3]
    assert (status == oh.RAY_HIT).mean() >= 0.2 and (status == oh.RAY_BODY).mean() >= 0.05 and np.isfinite(imgs[1]).all()
    plain = on.camera_bodies(cam, side, side, bodies, BOX, PAINT, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE)
    assert ((imgs[1] != plain).any(axis=-1) & (status == oh.RAY_HIT)).sum() >= 1000  # the links are in the picture
    for ctx in (off, on):
        ctx.close()


def test_forms_agree_over_the_state_of_body_step_device():
    """The device form over the `out` of ocean_body_step_device, stride 32, where it lies, equals the blocking form over
    the first ten floats of the landed records; the async form lands the same bytes, also behind later steps and with
    the caller's arrays overwritten; an async result larger than a slot is refused, and the blocking form serves it."""
    import torch
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    ctx, ref = make_ctx(n, cas, oh.F_VELOCITY, times=()), make_ctx(n, cas, oh.F_VELOCITY, times=())
    ref.step(times[0])
    ctx.step(times[0])
    cam, poses = scene(ref)
    count = len(poses)
    hull = oh.OceanContext.box_hull(2, 2)
    state = oh.OceanContext.body_state(poses)
    props = np.tile(f32([0.01, 0.02, 0.02, 0.02]), (count, 1))
    step = oh.step_params(1.0 / 120.0)
    dev = torch.device("cuda", ctx.device)
    d_hull, d_props, d_state = (torch.from_numpy(a).to(dev) for a in (hull, props, state))
    d_out = torch.zeros((count, 32), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.body_step_device(d_hull.data_ptr(), len(hull), d_props.data_ptr(), d_state.data_ptr(), count, d_out.data_ptr(), step,
                         substeps=2)
    mat = sun_material()
    imgs = {}
    for mode in (LINKS, oh.CAMERA_COLOR):
        o = torch.full((W * H * 4 + 4,), -1.0, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        ctx.camera_scene_device(o.data_ptr(), cam, W, H, d_out.data_ptr(), count, 32, BOX, PAINT, OPTICS, mode, mat, 0, K,
                                STEPS, REFINE)
        ctx.synchronize()
        imgs[mode] = o[:W * H * 4].cpu().numpy().reshape(H, W, 4)
        np.testing.assert_array_equal(o[W * H * 4:].cpu().numpy(), f32(-1))  # nothing past the image
    landed = d_out.cpu().numpy()
    assert not np.array_equal(landed[:, :10], poses)  # the bodies moved
    for mode in (LINKS, oh.CAMERA_COLOR):
        want = shoot(ctx, cam, np.ascontiguousarray(landed[:, :10]), mode, mat)
        np.testing.assert_array_equal(imgs[mode], want)
        np.testing.assert_array_equal(shoot(ctx, cam, landed, mode, mat), want)  # stride 32 from the host
        slot = oh.PinnedBuffer(W * H * 16)
        rb = ctx.camera_scene_async(cam, W, H, landed, BOX, PAINT, OPTICS, mode, mat, 0, K, STEPS, REFINE, buf=slot)
        np.testing.assert_array_equal(rb.data, want)
        rb.release()
        slot.release()
    _, info = restate_camera_scene(Textures(ctx, cas), cam, mat, W, H, LINKS, K, STEPS, REFINE, BOX, None, OPTICS,
                                   np.ascontiguousarray(landed[:, :10]))
    check_link_shares(info)
    # the async request made after step t1, with two more steps queued right behind it, holds the image of t1
    want = shoot(ref, cam, landed, oh.CAMERA_COLOR, mat)
    cbuf, mbuf, bbuf, xbuf, pbuf, obuf = cam.copy(), mat.copy(), landed.copy(), BOX.copy(), PAINT.copy(), OPTICS.copy()
    rb = ctx.camera_scene_async(cbuf, W, H, bbuf, xbuf, pbuf, obuf, oh.CAMERA_COLOR, mbuf, 0, K, STEPS, REFINE)
    for a in (cbuf, mbuf, bbuf, xbuf, pbuf, obuf):
        a[:] = 1.0e9
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    got = rb.data
    rb.release()
    np.testing.assert_array_equal(got, want)
    assert not np.array_equal(got, shoot(ctx, cam, landed, oh.CAMERA_COLOR, mat))  # frame t3
    # 416 x 416 pixels of 16 B = 2,768,896 B > a slot of max(256 * 256 * 16, 65536 * 40) = 2,621,440 B
    with pytest.raises(oh.OceanError) as e:
        ctx.camera_scene_async(cam, 416, 416, landed, BOX, PAINT, OPTICS, LINKS, mat, 0, K, 1, 0)
    assert e.value.code == oh.E_INVALID_ARG and "slot" in str(e.value) and "ocean_camera_scene_async" in str(e.value)
    assert ctx.camera_scene(cam, 416, 416, landed, BOX, PAINT, OPTICS, LINKS, mat, 0, 0, 1, 0).shape == (416, 416, 4)
    # a misaligned device `bodies`, and the state rule before ocean_init_spectrum
    L, vp = ctx.lib, ctypes.c_void_p
    o = torch.zeros(W * H * 4, dtype=torch.float32, device=dev)
    assert L.ocean_camera_scene_device(ctx._h, 0, LINKS, K, STEPS, REFINE, vp(cam.ctypes.data), vp(mat.ctypes.data), W, H,
                                       vp(BOX.ctypes.data), None, vp(OPTICS.ctypes.data), vp(d_out.data_ptr() + 2), 32, 4,
                                       vp(o.data_ptr()), W * H * 16) == oh.E_INVALID_ARG
    assert b"aligned" in L.ocean_last_error()
    ctx.close()
    ref.close()
    bare = oh.OceanContext(64, 2, 1)
    for call in (bare.camera_scene, bare.camera_scene_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, landed, BOX, PAINT, OPTICS, oh.CAMERA_COLOR, mat)
        assert e.value.code == oh.E_STATE and "ocean_init_spectrum" in str(e.value)
    bare.close()


def test_camera_scene_on_a_later_tile():
    """T = 2: tile 1's image is checked against tile 1's own textures, and tile 0's differs."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, tiles=2)
    cam, bodies = scene(ctx, tile=1)
    tex = Textures(ctx, cas, tile=1)
    mat = sun_material()
    want, info = restate_camera_scene(tex, cam, mat, W, H, LINKS, K, STEPS, REFINE, BOX, None, OPTICS, bodies)
    check_link_shares(info)
    got = shoot(ctx, cam, bodies, LINKS, mat, tile=1).reshape(-1, 4)
    np.testing.assert_array_equal(got, want)
    other = shoot(ctx, cam, bodies, LINKS, mat, tile=0).reshape(-1, 4)
    assert not np.array_equal(got, other)
    ctx.close()


def test_water_body_camera_scene_is_the_context_call():
    wb = oh.scene_water_body(n=64, n_cascades=2, readback="probes").Awake()
    wb.Update(0.5)
    eye, target = (3.0, 12.0, -4.0), (40.0, 4.0, 50.0)
    cam = oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 1.0, W, H, 0.0, 2000.0)
    bodies = scene_boxes(cam, wb.ctx.surface_bounds(), W, H)
    img = wb.camera_scene(eye, target, W, H, bodies, BOX, PAINT, OPTICS)
    assert img.shape == (H, W, 4) and (img[..., 3] == oh.RAY_BODY).any()
    np.testing.assert_array_equal(img, wb.ctx.camera_scene(cam, W, H, bodies, BOX, PAINT, OPTICS, oh.CAMERA_COLOR, oh.material()))
    links = wb.camera_scene(eye, target, W, H, bodies, BOX, None, OPTICS, mode=LINKS)
    np.testing.assert_array_equal(links[..., 3], img[..., 3])
    wb.OnDisable()
