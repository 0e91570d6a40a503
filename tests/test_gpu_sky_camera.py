"""GPU tests of the camera's OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT mode (csrc/view.hip, k_camera_sky) against
tests/atmosphere_ref.sky_colours, the numpy restatement of include/ocean/ocean.h over the context's own read-back
textures and its own sky-view table, so that the table's error does not compound.  The status channel is exact; the
colours meet the criterion of tests/test_gpu_atmosphere.py: per channel, the device's distance to the float64
restatement is at most 4 x the fp32 restatement's own.

The scene is one cascade at 64^2 and a 32 x 24 image (two workgroup tiles wide and two tall, the lower ones partial).
The camera stands a few metres over the highest crest, looks towards the sun and five degrees up: water in the lower
rows, sky in the upper ones, the sun's disc inside the frame."""
import numpy as np
import pytest

import atmosphere_ref as A
import ocean_hip as oh
import oracle as O
from test_camera_abi import shading_inputs
from test_gpu_query import Textures, make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
W, H, K, STEPS, REFINE = 32, 24, 2, 32, 6
SKY = oh.CAMERA_COLOR | oh.CAMERA_SKY_LUT
CAS = O.SCENE_CASCADES[:1]
SUN_UP = (0.3, 0.25, 0.9)       # about 15 degrees over the horizon
SUN_DOWN = (0.3, -0.05, 0.9)    # just under it: the sky is still lit, the sun's lobes are off
PARAMS = oh.atmosphere_params()


def pose_towards(bounds, sun, pitch_degrees=5.0):
    top = float(bounds[:, 5].astype(np.float64).sum())
    eye = np.float64([3.0, top + 4.0, -4.0])
    ahead = np.float64([sun[0], 0.0, sun[2]])
    ahead /= np.linalg.norm(ahead)
    target = eye + 100.0 * ahead + np.float64([0.0, 100.0 * np.tan(np.radians(pitch_degrees)), 0.0])
    return oh.look_at_camera(eye, target, (0.0, 1.0, 0.0), 0.9, W, H, 0.0, 400.0)


def sky_material(ctx, sun, **kw):
    return oh.material(roughness=0.3, light_direction=sun, light_color=ctx.sun_color(sun), **kw)


def check_image(ctx, tex, cam, mat, expect_disc):
    S = ctx.atmosphere_lut(oh.LUT_SKYVIEW)
    args = shading_inputs(tex, cam, mat, W, H, K, STEPS, REFINE)
    rec = args[1]
    want32, spot = A.sky_colours(*args, mat, tex.deriv is not None, S, PARAMS[26], f32)
    want64, _ = A.sky_colours(*args, mat, tex.deriv is not None, S, PARAMS[26], np.float64)
    status = rec[:, 3]
    hit, miss = (status == oh.RAY_HIT).mean(), (status == oh.RAY_MISS).mean()
    disc = (status == oh.RAY_MISS) & (spot > 0)
    print(f"hit {hit:.3f}, miss {miss:.3f}; {int(disc.sum())} miss pixels inside the sun's disc, largest spot {spot.max()}")
    assert hit >= 0.2 and miss >= 0.2
    assert disc.any() == expect_disc
    got = ctx.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    assert got.shape == (H, W, 4) and got.dtype == f32 and np.isfinite(got).all()
    got = got.reshape(-1, 4)
    np.testing.assert_array_equal(got[:, 3], status)
    for c in range(3):
        e_dev = np.linalg.norm(got[:, c].astype(np.float64) - want64[:, c])
        e_ref = np.linalg.norm(want32[:, c].astype(np.float64) - want64[:, c])
        print(f"channel {c}: |ref| {np.linalg.norm(want64[:, c]):.6g}, restatement error {e_ref:.3g}, device error "
              f"{e_dev:.3g}, ratio {e_dev / e_ref:.3f}")
        assert e_ref > 0 and e_dev <= 4.0 * e_ref, (c, e_dev, e_ref)
    if expect_disc:  # the disc is in the picture: those pixels are brighter than the sky beside them by spot^2 LC
        k = int(np.argmax(np.where(disc, spot, 0)))
        np.testing.assert_allclose(got[k, :3], A.sky_lookup(S, args[0][k:k + 1, 3:6], np.float64)[0]
                                   + np.float64(spot[k]) ** 2 * np.float64(mat[23:26]), rtol=1e-3)
    return got


def test_sky_mode_matches_the_restatement_with_the_sun_in_the_frame():
    ctx = make_ctx(64, CAS)
    tex = Textures(ctx, CAS)
    cam = pose_towards(ctx.surface_bounds(), SUN_UP)
    plain_mat = oh.material(roughness=0.3)
    before = ctx.camera(cam, W, H, oh.CAMERA_COLOR, plain_mat, 0, K, STEPS, REFINE)
    ctx.atmosphere()
    # the flag on a context whose sky-view table is stale: OCEAN_E_STATE, in every form, after the argument checks
    for call in (ctx.camera, ctx.camera_async):
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, SKY, plain_mat, 0, K, STEPS, REFINE)
        assert e.value.code == oh.E_STATE and "ocean_sky_update" in str(e.value)
        with pytest.raises(oh.OceanError) as e:
            call(cam, W, H, SKY, plain_mat, 0, K, 0, REFINE)
        assert e.value.code == oh.E_INVALID_ARG and "steps" in str(e.value)
    ctx.sky_update(SUN_UP)
    mat = sky_material(ctx, SUN_UP)
    got = check_image(ctx, tex, cam, mat, expect_disc=True)
    # material[26..31], the two-colour sky, are ignored by the mode
    other = mat.copy()
    other[26:32] = (9, 8, 7, 6, 5, 4)
    np.testing.assert_array_equal(ctx.camera(cam, W, H, SKY, other, 0, K, STEPS, REFINE).reshape(-1, 4), got)
    # OCEAN_CAMERA_COLOR on the same context is what it was before the atmosphere, bit for bit
    np.testing.assert_array_equal(ctx.camera(cam, W, H, oh.CAMERA_COLOR, plain_mat, 0, K, STEPS, REFINE), before)
    assert not np.array_equal(ctx.camera(cam, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE).reshape(-1, 4)[:, :3], got[:, :3])
    # from below the surface every pixel is the water colour
    low = float(ctx.surface_bounds()[:, 1].astype(np.float64).sum())
    eye = np.float64([-7.0, low - 3.0, 11.0])
    sub = oh.look_at_camera(eye, eye + np.float64([0.5, 0.4, -0.7]), (0.0, 1.0, 0.0), 0.9, W, H, 0.0, 50.0)
    col = ctx.camera(sub, W, H, SKY, mat, 0, K, STEPS, REFINE)
    np.testing.assert_array_equal(col.reshape(-1, 4), np.tile(np.r_[mat[0:3], f32(oh.RAY_SUBMERGED)], (W * H, 1)))
    ctx.close()


def test_sky_mode_with_the_sun_below_the_horizon():
    ctx = make_ctx(64, CAS)
    tex = Textures(ctx, CAS)
    ctx.atmosphere()
    ctx.sky_update(SUN_DOWN)
    mat = sky_material(ctx, SUN_DOWN)
    assert mat[21] < 0
    got = check_image(ctx, tex, pose_towards(ctx.surface_bounds(), SUN_DOWN), mat, expect_disc=False)
    assert (got[got[:, 3] == oh.RAY_MISS, :3] > 0).any()  # twilight: the sky is not black
    ctx.close()


def test_forms_agree_and_a_second_sun_equals_a_fresh_context():
    import torch
    ctx, ref = make_ctx(64, CAS), make_ctx(64, CAS)
    cam = pose_towards(ctx.surface_bounds(), SUN_UP)
    ctx.atmosphere()
    ctx.sky_update(SUN_UP)
    mat = sky_material(ctx, SUN_UP)
    first = ctx.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    # the three forms, bit for bit
    rb = ctx.camera_async(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    rb.wait()
    np.testing.assert_array_equal(rb.data, first)
    rb.release()
    o = torch.full((W * H * 4 + 4,), -1.0, dtype=torch.float32, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ctx.camera_device(o.data_ptr(), cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    ctx.synchronize()
    np.testing.assert_array_equal(o[:W * H * 4].cpu().numpy().reshape(first.shape), first)
    np.testing.assert_array_equal(o[W * H * 4:].cpu().numpy(), f32(-1))  # nothing past the image
    # sky_update(A), camera, sky_update(B), camera, all queued: the second image is a fresh context's
    ctx.sky_update(SUN_DOWN)
    second = ctx.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    ref.atmosphere()
    ref.sky_update(SUN_DOWN)
    np.testing.assert_array_equal(second, ref.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE))
    assert not np.array_equal(first, second)
    # a new ocean_atmosphere makes the table stale for the camera as well
    ctx.atmosphere()
    with pytest.raises(oh.OceanError) as e:
        ctx.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    assert e.value.code == oh.E_STATE
    # and a context that never had an atmosphere refuses the mode alone
    bare = make_ctx(64, CAS)
    with pytest.raises(oh.OceanError) as e:
        bare.camera(cam, W, H, SKY, mat, 0, K, STEPS, REFINE)
    assert e.value.code == oh.E_STATE
    assert bare.camera(cam, W, H, oh.CAMERA_COLOR, mat, 0, K, STEPS, REFINE).shape == (H, W, 4)
    for c in (ctx, ref, bare):
        c.close()
