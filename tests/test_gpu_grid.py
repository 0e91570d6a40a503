"""GPU tests of the surface grids (ocean_surface_grid / _device / _async, csrc/grid.hip).  The yardsticks are
the point entries over OceanContext.grid_points(...): ocean_query_surface for the surface and heightfield
modes and ocean_sample_world for the vertices, themselves tested against the oracle (tests/test_gpu_query.py,
tests/test_gpu_sample.py).  The grid kernel runs the same fp32 operations in the same order, so every
comparison is bit for bit."""
import ctypes
import math

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_query import make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
KS = (0, 1, 4, 16)
LODS = (0.0, 0.5, 2.25, 99.0)


def grids(n, cas):
    """(x0, z0, dx, dz, nx, ny): the smallest shapes that cross every edge of the kernel's mapping -- one node,
    one column, one row, partial tiles on both axes for each of the 64 x 4, 32 x 8 and 16 x 16 workgroup
    tiles -- then MeshGenerator's default plane, overlapping footprints (0.37 texels of the finest cascade, x
    running backwards) and a zero spacing."""
    texel = min(c["wavelength"] for c in cas) / n
    return [
        (3.25, -7.5, 1.0, 1.0, 1, 1),
        (-13.7, 5.3, 0.83, 1.21, 1, 70),
        (-13.7, 5.3, 0.83, 1.21, 70, 1),
        (120.0, -310.5, 2.9, 7.3, 67, 5),
        (-813.7, 405.3, 3.83, 11.21, 130, 37),
        (-500.0, -500.0, 10.0, 10.0, 101, 101),
        (17.0, -4.0, -0.37 * texel, 0.37 * texel, 80, 40),
        (-40.0, 12.5, 1.7, 0.0, 50, 20),
    ]


@pytest.mark.parametrize("n,ncasc,flags", [(64, 1, 0), (64, 4, 0), (256, 3, oh.F_DISPLACEMENT_ONLY)])
def test_grid_surface_and_heightfield_match_the_point_query(n, ncasc, flags):
    """GRID_SURFACE is ocean_query_surface over grid_points, GRID_HEIGHTFIELD its column 0, for K in
    {0, 1, 4, 16}; the (64, 4) scene is not contractive and must match all the same."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    for g in grids(n, cas):
        nx, ny = g[4], g[5]
        q = oh.OceanContext.grid_points(*g)
        assert len(q) <= oh.QUERY_MAX_POINTS
        for k in KS:
            want = ctx.query_surface(q, iterations=k).reshape(ny, nx, 8)
            got = ctx.surface_grid(*g, mode=oh.GRID_SURFACE, iterations=k)
            assert got.shape == (ny, nx, 8) and got.dtype == f32
            np.testing.assert_array_equal(got, want, err_msg=f"grid {g}, K = {k}")
            h = ctx.surface_grid(*g, mode=oh.GRID_HEIGHTFIELD, iterations=k)
            assert h.shape == (ny, nx) and h.dtype == f32
            np.testing.assert_array_equal(h, want[..., 0], err_msg=f"heightfield {g}, K = {k}")
            if k == 0:
                np.testing.assert_array_equal(got[..., 1:3].reshape(-1, 2), q)  # p_0 = q: the nodes themselves
    # the default arguments: surface mode, 4 steps
    g = grids(n, cas)[3]
    np.testing.assert_array_equal(ctx.surface_grid(*g), ctx.surface_grid(*g, mode=oh.GRID_SURFACE, iterations=4))
    ctx.close()


@pytest.mark.parametrize("n,ncasc,flags", [(128, 2, oh.F_MIPS), (64, 2, 0), (256, 3, oh.F_DISPLACEMENT_ONLY)])
def test_grid_vertices_match_world_sampling(n, ncasc, flags):
    """GRID_VERTICES is the domain stage over the plane: node + S.xz in fp32, S.y, the foam, the normal and a
    zero, with S = ocean_sample_world at (node, lod); lod 99 exercises the clamp to log2 N."""
    cas = O.SCENE_CASCADES[:ncasc]
    ctx = make_ctx(n, cas, flags)
    for g in grids(n, cas):
        nx, ny = g[4], g[5]
        q = oh.OceanContext.grid_points(*g)
        for lod in LODS:
            s = ctx.sample_world(np.concatenate([q, np.full((len(q), 1), lod, f32)], axis=1))
            got = ctx.surface_grid(*g, mode=oh.GRID_VERTICES, lod=lod)
            assert got.shape == (ny, nx, 8)
            got = got.reshape(-1, 8)
            msg = f"grid {g}, lod = {lod}"
            np.testing.assert_array_equal(got[:, [0, 2]], q + s[:, 0, [0, 2]], err_msg=msg)  # fp32 + fp32
            np.testing.assert_array_equal(got[:, 1], s[:, 0, 1], err_msg=msg)
            np.testing.assert_array_equal(got[:, 3], s[:, 0, 3], err_msg=msg)
            np.testing.assert_array_equal(got[:, 4:7], s[:, 2, :3], err_msg=msg)
            np.testing.assert_array_equal(got[:, 7], np.zeros(len(q), f32), err_msg=msg)
            if flags & oh.F_DISPLACEMENT_ONLY:
                np.testing.assert_array_equal(got[:, 3:], np.tile(f32([0, 0, 1, 0, 0]), (len(q), 1)))
    # iterations default to 0 in this mode, and the levels matter where the context has them
    g = grids(n, cas)[4]
    a = ctx.surface_grid(*g, mode=oh.GRID_VERTICES, iterations=0, lod=2.25)
    assert (not np.array_equal(a, ctx.surface_grid(*g, mode=oh.GRID_VERTICES))) == bool(flags & oh.F_MIPS)
    ctx.close()


@pytest.mark.parametrize("tile_w", ["64", "32", "16", "7"])
def test_grid_every_workgroup_tile_gives_the_same_bits(tile_w, monkeypatch):
    """OCEAN_GRID_TILE (read in ocean_create) maps nodes to lanes as 64 x 4, 32 x 8 or 16 x 16; any other value
    selects the default.  A mapping only: every shape gives the point entries' bits on every grid."""
    n, cas = 64, O.SCENE_CASCADES[:4]
    monkeypatch.setenv("OCEAN_GRID_TILE", tile_w)
    ctx = make_ctx(n, cas)
    for g in grids(n, cas):
        nx, ny = g[4], g[5]
        q = oh.OceanContext.grid_points(*g)
        want = ctx.query_surface(q, iterations=4).reshape(ny, nx, 8)
        np.testing.assert_array_equal(ctx.surface_grid(*g, mode=oh.GRID_SURFACE, iterations=4), want, err_msg=str(g))
        np.testing.assert_array_equal(ctx.surface_grid(*g, mode=oh.GRID_HEIGHTFIELD, iterations=4), want[..., 0])
        s = ctx.sample_world(np.concatenate([q, np.zeros((len(q), 1), f32)], axis=1))
        v = ctx.surface_grid(*g, mode=oh.GRID_VERTICES).reshape(-1, 8)
        np.testing.assert_array_equal(v[:, 1], s[:, 0, 1], err_msg=str(g))
        np.testing.assert_array_equal(v[:, 4:7], s[:, 2, :3], err_msg=str(g))
    ctx.close()


def test_grid_flat_sea_known_answer():
    """Zero noise: no waves.  The vertices are the nodes at y = 0 with the normal (0, 1, 0); heights are 0."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, noise=np.zeros((n, n, 2), f32))
    g = (-813.7, 405.3, 3.83, 11.21, 130, 37)
    q = oh.OceanContext.grid_points(*g)
    v = ctx.surface_grid(*g, mode=oh.GRID_VERTICES).reshape(-1, 8)
    want = np.zeros((len(q), 8), f32)
    want[:, 0], want[:, 2], want[:, 5] = q[:, 0], q[:, 1], 1.0
    np.testing.assert_array_equal(np.delete(v, 3, axis=1), np.delete(want, 3, axis=1))  # (all but the foam)
    for k in (0, 4):
        np.testing.assert_array_equal(ctx.surface_grid(*g, mode=oh.GRID_HEIGHTFIELD, iterations=k),
                                      np.zeros((37, 130), f32))
        s = ctx.surface_grid(*g, mode=oh.GRID_SURFACE, iterations=k).reshape(-1, 8)
        np.testing.assert_array_equal(s[:, 0], np.zeros(len(q), f32))
        np.testing.assert_array_equal(s[:, 1:3], q)
        np.testing.assert_array_equal(s[:, 4:7], np.tile(f32([0, 1, 0]), (len(q), 1)))
    ctx.close()


def test_grid_tiles():
    """A 2-tile context with different noise per tile: tile=1 answers from tile 1's textures."""
    n, cas = 64, O.SCENE_CASCADES[:2]
    ctx = make_ctx(n, cas, tiles=2)
    g = (120.0, -310.5, 2.9, 7.3, 67, 5)
    q = oh.OceanContext.grid_points(*g)
    a0 = ctx.surface_grid(*g, tile=0)
    a1 = ctx.surface_grid(*g, tile=1)
    np.testing.assert_array_equal(a0.reshape(-1, 8), ctx.query_surface(q, tile=0))
    np.testing.assert_array_equal(a1.reshape(-1, 8), ctx.query_surface(q, tile=1))
    assert not np.array_equal(a0[..., 0], a1[..., 0])
    np.testing.assert_array_equal(ctx.surface_grid(*g, mode=oh.GRID_HEIGHTFIELD, tile=1), a1[..., 0])
    v1 = ctx.surface_grid(*g, mode=oh.GRID_VERTICES, tile=1).reshape(-1, 8)
    s1 = ctx.sample_world(np.concatenate([q, np.zeros((len(q), 1), f32)], axis=1), tile=1)
    np.testing.assert_array_equal(v1[:, 1], s1[:, 0, 1])
    assert not np.array_equal(v1[:, 1], ctx.surface_grid(*g, mode=oh.GRID_VERTICES, tile=0).reshape(-1, 8)[:, 1])
    ctx.close()


def test_grid_async_snapshots_behind_later_steps():
    """ocean_surface_grid_async: the request made after step t1, with two more steps queued right behind it,
    holds the grid of t1 (a second context gives it), not that of t3; once more as a height map into a
    caller-owned pinned slot."""
    n, cas = 256, O.SCENE_CASCADES[:2]
    times = (0.25, 0.5, 0.75)
    g = (-813.7, 405.3, 3.83, 11.21, 130, 37)
    for mode, slot in ((oh.GRID_SURFACE, None), (oh.GRID_HEIGHTFIELD, oh.PinnedBuffer(130 * 37 * 4))):
        ctx, ref = make_ctx(n, cas, times=()), make_ctx(n, cas, times=())
        ctx.step(times[0])
        rb = ctx.surface_grid_async(*g, mode=mode, buf=slot)
        ctx.step(times[1])
        ctx.step(times[2])
        rb.wait()
        assert rb.done()
        got = rb.data
        rb.release()
        ref.step(times[0])
        want = ref.surface_grid(*g, mode=mode)
        assert got.shape == want.shape
        np.testing.assert_array_equal(got, want)
        later = ctx.surface_grid(*g, mode=mode)  # the blocking grid now: frame t3
        np.testing.assert_array_equal(later[..., 0] if mode == oh.GRID_SURFACE else later,
                                      ctx.query_surface(oh.OceanContext.grid_points(*g))[:, 0].reshape(37, 130))
        assert not np.array_equal(got, later)
        if slot is not None:
            slot.release()
        ctx.close()
        ref.close()


class Forms:
    """The three C entries called directly, with every argument overridable: what the Python methods cannot
    pass (a wrong byte count, a null or misaligned pointer)."""

    DEFAULT = dict(tile=0, mode=oh.GRID_SURFACE, iterations=4, lod=0.0, x0=0.0, z0=0.0, dx=1.0, dz=1.0, nx=4, ny=4)

    def __init__(self, ctx):
        import torch
        self.ctx, self.lib = ctx, ctx.lib
        self.host = np.zeros(4096, f32)
        self.pinned = oh.PinnedBuffer(4096 * 4)
        self.dev = torch.zeros(4096, dtype=torch.float32, device=torch.device("cuda", ctx.device))
        torch.cuda.synchronize()

    def call(self, form, **kw):
        """-> (status, request handle or None)."""
        a = dict(self.DEFAULT, **{k: v for k, v in kw.items() if k not in ("bytes", "out")})
        nbytes = kw.get("bytes", a["nx"] * a["ny"] * (4 if a["mode"] == oh.GRID_HEIGHTFIELD else 32))
        out = {"host": self.host.ctypes.data, "device": self.dev.data_ptr(), "async": self.pinned.ptr.value}[form]
        out = kw.get("out", out)
        args = (self.ctx._h, a["tile"], a["mode"], a["iterations"], a["lod"], a["x0"], a["z0"], a["dx"], a["dz"],
                a["nx"], a["ny"], ctypes.c_void_p(out), ctypes.c_size_t(nbytes))
        if form == "host":
            return self.lib.ocean_surface_grid(*args), None
        if form == "device":
            return self.lib.ocean_surface_grid_device(*args), None
        req = ctypes.c_void_p(0x1234)
        rc = self.lib.ocean_surface_grid_async(*args, ctypes.byref(req))
        return rc, req.value

    def release(self):
        self.pinned.release()


BAD = [dict(tile=1), dict(tile=-1), dict(mode=3), dict(mode=-1), dict(iterations=17), dict(iterations=-1),
       dict(mode=oh.GRID_VERTICES, iterations=1), dict(lod=math.nan), dict(lod=math.inf), dict(lod=-0.5),
       dict(mode=oh.GRID_VERTICES, iterations=0, lod=-1.0), dict(mode=oh.GRID_VERTICES, iterations=0, lod=math.nan),
       dict(mode=oh.GRID_SURFACE, lod=0.5), dict(mode=oh.GRID_HEIGHTFIELD, lod=0.5),
       dict(x0=math.nan), dict(x0=math.inf), dict(z0=math.nan), dict(z0=-math.inf),
       dict(dx=math.nan), dict(dx=math.inf), dict(dz=math.nan), dict(dz=-math.inf),
       dict(nx=0), dict(ny=0), dict(nx=-4), dict(ny=-1),
       dict(nx=2049, ny=2048), dict(nx=2049, ny=2048, mode=oh.GRID_HEIGHTFIELD), dict(nx=1 << 16, ny=1 << 16),
       dict(bytes=4 * 4 * 32 - 4), dict(bytes=4 * 4 * 32 + 32), dict(bytes=4 * 4 * 4), dict(bytes=0),
       dict(mode=oh.GRID_HEIGHTFIELD, bytes=4 * 4 * 32), dict(out=None)]


def test_grid_errors_and_device_form():
    import torch
    # OCEAN_E_STATE before ocean_init_spectrum, after the argument checks
    ctx = oh.OceanContext(64, 2, 1)
    forms = Forms(ctx)
    for form in ("host", "device", "async"):
        assert forms.call(form) == (oh.E_STATE, None), form
        assert forms.call(form, mode=7) == (oh.E_INVALID_ARG, None), form
    with pytest.raises(oh.OceanError) as e:
        ctx.surface_grid(0.0, 0.0, 1.0, 1.0, 4, 4)
    assert e.value.code == oh.E_STATE
    with pytest.raises(oh.OceanError) as e:
        ctx.surface_grid_async(0.0, 0.0, 1.0, 1.0, 4, 4)
    assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    # every OCEAN_E_INVALID_ARG case, for all three forms; the async form hands back no request
    for kw in BAD:
        for form in ("host", "device", "async"):
            assert forms.call(form, **kw) == (oh.E_INVALID_ARG, None), (form, kw)
            assert ctx.lib.ocean_last_error(), (form, kw)
    assert ctx.lib.ocean_surface_grid_async(ctx._h, 0, oh.GRID_SURFACE, 4, 0.0, 0.0, 0.0, 1.0, 1.0, 4, 4,
                                            forms.pinned.ptr, 4 * 4 * 32, None) == oh.E_INVALID_ARG  # req null
    # ... through the Python methods as well
    for kw in (dict(mode=5), dict(iterations=17), dict(lod=0.5), dict(tile=1)):
        for call in (ctx.surface_grid, ctx.surface_grid_async):
            with pytest.raises(oh.OceanError) as e:
                call(0.0, 0.0, 1.0, 1.0, 4, 4, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
    for call in (ctx.surface_grid, ctx.surface_grid_async):
        with pytest.raises(oh.OceanError) as e:
            call(0.0, 0.0, 1.0, 1.0, 2049, 2048, mode=oh.GRID_HEIGHTFIELD)  # GRID_MAX_NODES + 2048 nodes
        assert e.value.code == oh.E_INVALID_ARG
    # zero and negative spacings are valid
    for kw in (dict(dx=0.0, dz=0.0), dict(dx=-1.0, dz=-2.5)):
        assert forms.call("host", **kw) == (oh.OK, None), kw
    # the async capacity at N = 64: a slot is max(64 * 64 * 16, 65536 * 40) = 2,621,440 B
    g = (-37.0, 21.0, 0.25, 0.25, 300, 300)
    with pytest.raises(oh.OceanError) as e:
        ctx.surface_grid_async(*g, mode=oh.GRID_SURFACE)  # 2,880,000 B
    assert e.value.code == oh.E_INVALID_ARG
    rb = ctx.surface_grid_async(*g, mode=oh.GRID_HEIGHTFIELD)  # 360,000 B
    np.testing.assert_array_equal(rb.data, ctx.surface_grid(*g, mode=oh.GRID_HEIGHTFIELD))
    rb.release()
    # the device form: async on the ctx stream, and a misaligned pointer is refused, not faulted on
    g = (120.0, -310.5, 2.9, 7.3, 67, 5)
    dev = torch.device("cuda", ctx.device)
    for mode, per in ((oh.GRID_SURFACE, 8), (oh.GRID_VERTICES, 8), (oh.GRID_HEIGHTFIELD, 1)):
        count = 67 * 5 * per
        o = torch.zeros(count + 4, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        it = 0 if mode == oh.GRID_VERTICES else 4
        args = (ctx._h, 0, mode, it, 0.0, *g[:4], 67, 5)
        for off in (4, 8, 12):
            assert ctx.lib.ocean_surface_grid_device(*args, ctypes.c_void_p(o.data_ptr() + off),
                                                     count * 4) == oh.E_INVALID_ARG
        assert ctx.lib.ocean_surface_grid_device(*args, ctypes.c_void_p(o.data_ptr()), count * 4) == oh.OK
        ctx.synchronize()
        got = o.cpu().numpy()
        np.testing.assert_array_equal(got[:count], ctx.surface_grid(*g, mode=mode).ravel())
        np.testing.assert_array_equal(got[count:], np.zeros(4, f32))  # nothing past the last node
    forms.release()
    ctx.close()
    # a column-parity shard holds half the columns: unsupported, as the queries
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    forms = Forms(par)
    for form in ("host", "device", "async"):
        assert forms.call(form) == (oh.E_UNSUPPORTED, None), form
    forms.release()
    par.close()
