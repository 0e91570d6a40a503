"""Deferred TURB (frame_plan.h defer_turb): a context whose frames are all pass BQ stores the 4-B foam state only and
writes the TURB float4 array when an entry shows it.

The reference object everywhere is an eager twin: the same context, same scene, noise and knobs, whose TURB pointer
ocean_get_device_ptr handed out before the first step, so that every frame of it writes TURB with the kernels this
library had before TURB could be deferred.  Every comparison is np.array_equal: the deferred kernel is the eager
one without a store, the materialise kernel copies the foam state, and the consumers' taps of the state run tap_x's
operations on the same values (sample_filter.h).

Shapes, all N = 512 (the smallest size pass BQ is built for) x 2 cascades: dense; one band-limited cascade (the
PRUNE instantiation); two tiles; OCEAN_TILE_W=4 and 16; OCEAN_MAX_GROUPS capped, so that a workgroup loops over
several items.  These jobs have fewer column tiles than the part has CUs, so ocean_create gives them 4-column
tiles by itself and OCEAN_TILE_W=16 is the case that runs the size's own width: the foam state is tile-major
[N/4][N][4] in every shape but tile_w16, where it is [N/16][N][16].  assert_modes reads the width off the kernel's
WT argument (4, or 0 for the size's own), so each case shows which layout it ran."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_camera import H, W, pose_above
from test_gpu_parity import _ctx_with_env
from test_gpu_prune import DENSE, SPARSE

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

N = 512
TIMES = (0.0, 0.5, 250.0)
MATERIALISE = "k_turb_materialise"
SHAPES = {
    "dense": ({}, [DENSE, O.SCENE_CASCADES[1]], 1),
    "prune": ({}, [DENSE, SPARSE], 1),
    "tiles2": ({}, [DENSE, O.SCENE_CASCADES[1]], 2),
    "tile_w4": ({"OCEAN_TILE_W": "4"}, [DENSE, O.SCENE_CASCADES[1]], 1),
    "tile_w16": ({"OCEAN_TILE_W": "16"}, [DENSE, O.SCENE_CASCADES[1]], 1),
    "capped": ({"OCEAN_MAX_GROUPS": "3"}, [DENSE, SPARSE], 1),
}
shapes = pytest.mark.parametrize("shape", list(SHAPES))


def twins(shape, flags=0):
    """(deferred, eager, tiles): two contexts that differ in the TURB pointer taken before the first step alone."""
    env, cas, tiles = SHAPES[shape]
    d, _ = _ctx_with_env(env, N, cas, tiles=tiles, flags=flags)
    e, _ = _ctx_with_env(env, N, cas, tiles=tiles, flags=flags)
    ptr, nbytes = e.device_ptr(oh.TEX_TURB)
    assert ptr and nbytes == tiles * len(cas) * N * N * 16
    return d, e, tiles


def step_both(d, e, times):
    for t in times:
        d.step(t)
        e.step(t)


def assert_modes(d, e, shape):
    """The deferred context ran the kernel without the TURB store, its twin the kernel with it, same arguments;
    WT = 0 (16-column tiles) in the tile_w16 shape and 4 in every other."""
    kd, ke = d.kernel_name(1), e.kernel_name(1)
    wt = 0 if shape == "tile_w16" else 4
    assert f"turb_deferred::k_pass_bq<512, false, {wt}," in kd, kd
    assert "k_pass_bq<512, false," in ke and "turb_deferred" not in ke, ke
    assert kd.replace("turb_deferred::", "") == ke, (kd, ke)


def assert_textures(d, e, tiles, what):
    for tile in range(tiles):
        for tex in (oh.TEX_TURB, oh.TEX_DISP, oh.TEX_DERIV):
            assert np.array_equal(d.read_all(tex, tile), e.read_all(tex, tile)), f"{what}: texture {tex}, tile {tile}"


def other_launches(ctx):
    """Launches of kind 2 since the last call, and the last kernel of that kind."""
    count = ctx.kernel_stats(2)[1]
    return count, (ctx.kernel_name(2) or "")


def peek(ctx, ptr, nbytes):
    """The bytes behind a device pointer once the context's stream has drained, with no other call on the context."""
    import torch
    torch.cuda.init()
    hip = ctypes.CDLL("libamdhip64.so.7", mode=ctypes.RTLD_GLOBAL | getattr(ctypes, "RTLD_NOLOAD", 4))
    ctx.synchronize()
    out = np.empty(nbytes // 4, np.float32)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    assert hip.hipMemcpy(out.ctypes.data, ptr, nbytes, 2) == 0
    return out


@shapes
def test_reads_and_launches(shape):
    """read(TURB) after three steps; read, step, read again; read_async.  A context that only steps launches no
    kernel of kind 2; the first read launches the materialise kernel once, a second read without a step not at
    all, and a read after the next step once again."""
    d, e, tiles = twins(shape)
    d.set_kernel_timing(True)
    step_both(d, e, TIMES)
    assert_modes(d, e, shape)
    assert other_launches(d)[0] == 0
    first = d.read(oh.TEX_TURB, tiles - 1, 1)
    assert other_launches(d) == (1, d.kernel_name(2)) and MATERIALISE in d.kernel_name(2)
    assert np.array_equal(first, e.read(oh.TEX_TURB, tiles - 1, 1))
    assert np.array_equal(first[..., 0], first[..., 3]) and first.any()
    assert_textures(d, e, tiles, "after three steps")
    assert other_launches(d)[0] == 0
    step_both(d, e, (250.5,))
    rb_d, rb_e = d.read_async(oh.TEX_TURB, 0, 1), e.read_async(oh.TEX_TURB, 0, 1)
    assert np.array_equal(rb_d.data, rb_e.data) and not np.array_equal(rb_d.data, first)
    assert other_launches(d)[0] == 1
    assert_textures(d, e, tiles, "read, step, read again")
    assert other_launches(d)[0] == 0
    d.close()
    e.close()


@shapes
def test_write_reset_reinit_pointer(shape):
    """ocean_write(TURB) of one slice, then a step: all slices and the next frame.  reset_foam.  A re-init keeps
    TURB.  The pointer taken mid-run: the array is whole at once, and after two more steps, now written by the
    eager kernel."""
    d, e, tiles = twins(shape)
    step_both(d, e, TIMES[:2])
    rng = np.random.default_rng(7)
    plant = np.repeat(rng.random((N, N, 1), np.float32), 4, axis=2)
    for c in (d, e):
        c.write(oh.TEX_TURB, plant, tiles - 1, 0)
    assert_textures(d, e, tiles, "after ocean_write(TURB)")
    assert np.array_equal(d.read(oh.TEX_TURB, tiles - 1, 0), plant)
    step_both(d, e, (1.0,))
    assert_textures(d, e, tiles, "the frame after ocean_write(TURB)")
    for c in (d, e):
        c.reset_foam()
    assert not d.read_all(oh.TEX_TURB).any()
    assert_textures(d, e, tiles, "after reset_foam")
    step_both(d, e, (1.5, 2.0))
    for c in (d, e):
        c.init_spectrum()
    assert_textures(d, e, tiles, "after a re-init")
    step_both(d, e, (2.5,))
    assert_modes(d, e, shape)
    ptr, nbytes = d.device_ptr(oh.TEX_TURB)
    whole = peek(d, ptr, nbytes).reshape(tiles, -1, N, N, 4)
    for tile in range(tiles):
        assert np.array_equal(whole[tile], e.read_all(oh.TEX_TURB, tile)), f"through the pointer, tile {tile}"
    step_both(d, e, (3.0, 3.5))
    assert d.kernel_name(1) == e.kernel_name(1) and "turb_deferred" not in d.kernel_name(1)
    whole = peek(d, ptr, nbytes).reshape(tiles, -1, N, N, 4)
    for tile in range(tiles):
        assert np.array_equal(whole[tile], e.read_all(oh.TEX_TURB, tile)), f"two steps after the pointer, tile {tile}"
    assert_textures(d, e, tiles, "two steps after the pointer")
    d.close()
    e.close()


@pytest.mark.parametrize("flags", [0, oh.F_MIPS], ids=["nomips", "mips"])
@shapes
def test_consumers(shape, flags):
    """The consumers of a deferred context tap the foam state: ocean_sample_world at lod 0, 0.5 and 2, a surface
    query, a vertex grid, whitecaps and a colour image equal the eager twin's, with and without mip chains, and so
    do levels 1 and last of TURB's chain.  Both twins launch the same number of kind-2 kernels over the sequence:
    the deferred one never materialises."""
    d, e, tiles = twins(shape, flags)
    tile = tiles - 1
    for c in (d, e):
        c.set_kernel_timing(True)
    step_both(d, e, TIMES)
    assert_modes(d, e, shape)
    rng = np.random.default_rng(11)
    xz = (rng.random((2048, 2)) * 3000.0 - 1500.0).astype(np.float32)
    bounds = e.surface_bounds(tile)
    assert np.array_equal(d.surface_bounds(tile), bounds)
    cam, mat = pose_above(bounds), oh.material(lod_slope=0.02)
    region = (-40.0, -25.0, 0.37, 0.41, 96, 64)
    out = {}
    for name, c in (("deferred", d), ("eager", e)):
        r = out[name] = {}
        for lod in (0.0, 0.5, 2.0):
            pts = np.concatenate([xz, np.full((len(xz), 1), lod, np.float32)], axis=1)
            r["sample", lod] = c.sample_world(pts, tile)
            r["grid", lod] = c.surface_grid(*region, mode=oh.GRID_VERTICES, lod=lod, tile=tile)
            thr = float(np.median(out["deferred"]["grid", lod][..., 3]))
            r["whitecaps", lod] = c.whitecaps(thr, *region, capacity=4096, lod=lod, tile=tile)
        r["query"] = c.query_surface(xz, tile)
        r["camera"] = c.camera(cam, W, H, oh.CAMERA_COLOR, mat, tile)
        if flags & oh.F_MIPS:
            for level in (1, int(np.log2(N))):
                r["mip", level] = c.read_mip(oh.TEX_TURB, level, tile, 1)
    for key, got in out["deferred"].items():
        want = out["eager"][key]
        if key[0] == "whitecaps":
            assert got[0] == want[0] and got[0] > 0 and np.array_equal(got[1], want[1]), key
        else:
            assert np.array_equal(got, want), key
    assert out["eager"]["sample", 0.0][:, 0, 3].std() > 0  # the foam the comparison is about is not constant
    nd, kd = other_launches(d)
    ne, _ = other_launches(e)
    assert nd == ne and MATERIALISE not in kd, (nd, ne, kd)
    assert_textures(d, e, tiles, "after the consumers")
    assert other_launches(d)[0] == 1
    d.close()
    e.close()


def test_knob_and_never_deferred():
    """OCEAN_DEFER_TURB=0 and a context after ocean_write(H0) (four-plane frames) run the eager kernels and never
    launch the materialise kernel; the first frame after the H0 upload starts from a whole array."""
    env, cas, tiles = SHAPES["dense"]
    k, _ = _ctx_with_env(dict(env, OCEAN_DEFER_TURB="0"), N, cas, tiles=tiles)
    d, e, _ = twins("dense")
    for c in (k, d, e):
        c.set_kernel_timing(True)
    for t in TIMES:
        k.step(t)
    step_both(d, e, TIMES)
    assert k.kernel_name(1) == e.kernel_name(1)
    assert other_launches(k)[0] == 0
    assert_textures(k, e, tiles, "OCEAN_DEFER_TURB=0")
    assert other_launches(k)[0] == 0
    h0 = d.read(oh.TEX_H0, 0, 0)
    for c in (d, e):
        c.write(oh.TEX_H0, h0, 0, 0)
    step_both(d, e, (251.0,))
    assert d.kernel_name(1) == e.kernel_name(1) and "k_pass_bq" not in d.kernel_name(1)
    assert other_launches(d) == (1, d.kernel_name(2)) and MATERIALISE in d.kernel_name(2)
    assert_textures(d, e, tiles, "the four-plane frame after ocean_write(H0)")
    assert other_launches(d)[0] == 0
    for c in (k, d, e):
        c.close()
