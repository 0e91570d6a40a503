"""GPU tests of the tile axis of the point consumers: ocean_sample_world, ocean_query_surface, ocean_surface_grid,
ocean_body_buoyancy and ocean_query_velocity with tile > 0.  Every entry, for every tile of a context whose tiles
hold different water, is compared bit for bit with its numpy fp32 restatement (oracle.sample_world, and
restate_surface / restate_reference / restate_body / restate_velocity of the sibling test files) over the
textures read back from that tile.  The shapes (T, C) = (3, 2) and (2, 3) put tile 1's slices at {2, 3} and
{3, 4, 5}, where the mappings tile + c ({1, 2}; {1, 2, 3}) and c T + tile ({1, 4}; {1, 3, 5}) stay in bounds
and land elsewhere; every slice is first asserted to differ from every other, so an answer from another slice
cannot pass."""
import ctypes
import itertools

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_body import (max_height, random_bodies, random_hull, reference_lookup, restate_body, surface_lookup)
from test_gpu_query import KS, Textures, make_ctx, restate_reference, restate_surface
from test_gpu_sample import _mips, _points
from test_gpu_velocity import restate_velocity

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
V = oh.F_VELOCITY
SHAPES = [(64, 3, 2, 0), (64, 2, 3, 0), (128, 3, 2, oh.F_MIPS)]  # (N, T, C, flags)
IDS = ["64-T3-C2", "64-T2-C3", "128-T3-C2-mips"]
GRID = (120.0, -310.5, 2.9, 7.3, 67, 5)
BODY_PROBES = (1, 37, 130)  # W = 1; W = 64 with a partial wave; more than one chunk
BODIES = 37


class World:
    """A T-tile context after two steps and, per tile, what the restatements take: the tile's textures, its
    mip chains (F_MIPS) and its VEL (F_VELOCITY), each read back once."""

    def __init__(self, n, tiles, ncasc, flags):
        self.n, self.T, self.C, self.flags = n, tiles, ncasc, flags
        self.cas = O.SCENE_CASCADES[:ncasc]
        self.lengths = [c["wavelength"] for c in self.cas]
        self.ctx = make_ctx(n, self.cas, flags, tiles=tiles)
        self.tex = [Textures(self.ctx, self.cas, t) for t in range(tiles)]
        self.mips = bool(flags & oh.F_MIPS)
        self.deriv_mips = [_mips(self.ctx, oh.TEX_DERIV, ncasc, t) if self.mips else None for t in range(tiles)]
        self.turb_mips = [_mips(self.ctx, oh.TEX_TURB, ncasc, t) if self.mips else None for t in range(tiles)]
        self.vel = [self.ctx.read_all(oh.TEX_VELOCITY, t) if flags & V else None for t in range(tiles)]

    def sample(self, t, pts):
        """O.sample_world over tile t's textures and, where the context has them, its mip chains."""
        x = self.tex[t]
        return O.sample_world(x.disp, x.deriv, x.turb, self.lengths, pts, self.deriv_mips[t], self.turb_mips[t])

    def queries(self, t):
        return np.ascontiguousarray(_points(4096, self.n, 100 * self.n + 10 * self.C + t)[:, :2])


@pytest.fixture(scope="module", params=SHAPES, ids=IDS)
def world(request, require_gpu):
    w = World(*request.param)
    yield w
    w.ctx.close()


@pytest.fixture(scope="module", params=SHAPES[:2], ids=IDS[:2])
def vworld(request, require_gpu):
    n, tiles, ncasc, flags = request.param
    w = World(n, tiles, ncasc, flags | V)
    yield w
    w.ctx.close()


@pytest.fixture(scope="module")
def world3(require_gpu):
    """The (T, C) = (3, 2) context at N = 64 once more, for the tests that take one shape."""
    w = World(*SHAPES[0])
    yield w
    w.ctx.close()


@pytest.fixture(scope="module")
def vworld3(require_gpu):
    n, tiles, ncasc, flags = SHAPES[0]
    w = World(n, tiles, ncasc, flags | V)
    yield w
    w.ctx.close()


def assert_slices_differ(w):
    """The precondition: every slice (tile, cascade) of DISP, DERIV and TURB differs from every other slice --
    so from the same cascade of every other tile, and from wherever a wrong slice index could land -- and so
    do the level-1 mips and VEL where the context has them."""
    slices = list(itertools.product(range(w.T), range(w.C)))
    for (ta, ca), (tb, cb) in itertools.combinations(slices, 2):
        what = f"slices ({ta}, {ca}) and ({tb}, {cb})"
        assert not np.array_equal(w.tex[ta].disp[ca], w.tex[tb].disp[cb]), f"DISP {what}"
        assert not np.array_equal(w.tex[ta].deriv[ca], w.tex[tb].deriv[cb]), f"DERIV {what}"
        assert not np.array_equal(w.tex[ta].turb[ca], w.tex[tb].turb[cb]), f"TURB {what}"
        if w.mips:
            assert not np.array_equal(w.deriv_mips[ta][ca][0], w.deriv_mips[tb][cb][0]), f"DERIV level 1 {what}"
            assert not np.array_equal(w.turb_mips[ta][ca][0], w.turb_mips[tb][cb][0]), f"TURB level 1 {what}"
        if w.vel[0] is not None:
            assert not np.array_equal(w.vel[ta][ca], w.vel[tb][cb]), f"VEL {what}"


def test_every_slice_differs(world):
    assert_slices_differ(world)


def test_every_slice_differs_velocity(vworld):
    assert_slices_differ(vworld)


def test_sample_world_every_tile(world):
    """ocean_sample_world(tile = t) is O.sample_world over tile t's textures and mip chains.  With F_MIPS the
    lod runs over [0, log2 N + 1]: levels >= 1 of the later tiles' chains, and the clamp."""
    w = world
    logn = w.n.bit_length() - 1
    for t in range(w.T):
        pts = _points(4096, w.n, 7 * w.n + w.C + t, lod_max=logn + 1.0 if w.mips else 3.0)
        if w.mips:
            assert ((pts[:, 2] >= 1.0) & (pts[:, 2] < logn)).any() and (pts[:, 2] > logn).any()
            pts[4:8, 2] = 0.0  # ... and level 0 of a context with chains
        got = w.ctx.sample_world(pts, tile=t)
        np.testing.assert_array_equal(got, w.sample(t, pts), err_msg=f"tile {t}")


def test_query_surface_every_tile(world):
    """ocean_query_surface(tile = t) is restate_surface over tile t's textures for K in {0, 1, 4, 16}; the
    reference mode is GetWaterHeight's texel of (t, cascade 0), at points across [-N/2 - 3, N/2 + 3]."""
    w = world
    for t in range(w.T):
        q = w.queries(t)
        want = restate_surface(w.tex[t], q, KS)
        for k in KS:
            got = w.ctx.query_surface(q, tile=t, iterations=k)
            np.testing.assert_array_equal(got, want[k], err_msg=f"tile {t}, K = {k}")
        rng = np.random.default_rng(31 * w.n + t)
        qr = rng.uniform(-w.n / 2 - 3, w.n / 2 + 3, (4096, 2)).astype(f32)
        got = w.ctx.query_surface(qr, tile=t, mode=oh.QUERY_REFERENCE, iterations=0)
        np.testing.assert_array_equal(got, restate_reference(w.tex[t].disp[0], qr), err_msg=f"tile {t}, reference mode")


def body_case(w, t, probes):
    """The hull and the poses of one (tile, P) case, scaled by the tile's own wave height
    (test_gpu_body.test_body_matches_restatement), and the same bodies moved over GetWaterHeight's window
    [-N/2 - 3, N/2 + 3] for the reference mode."""
    size = max_height(w.tex[t].disp)
    assert size > 0.0
    rng = np.random.default_rng(1000 * w.n + 100 * w.C + 10 * t + probes)
    hull, bodies = random_hull(rng, probes, size), random_bodies(rng, BODIES, size)
    near = bodies.copy()
    near[:, [0, 2]] = rng.uniform(-w.n / 2 - 3, w.n / 2 + 3, (BODIES, 2))
    return hull, bodies, near


def assert_shares(f, what):
    """The existing shares (test_body_matches_restatement): a quarter of the probes partly submerged, 5 % dry,
    5 % full, so the clamp of the submerged fraction cannot hide a wrong height."""
    partial, dry, full = ((f > 0) & (f < 1)).mean(), (f == 0).mean(), (f == 1).mean()
    print(f"{what}: {len(f)} probes, partly submerged {partial:.3f}, dry {dry:.3f}, full {full:.3f}")
    assert partial >= 0.25 and dry >= 0.05 and full >= 0.05, what


def test_body_buoyancy_every_tile(world):
    """ocean_body_buoyancy(tile = t) is restate_body over tile t's textures: P in {1, 37, 130} at K = 4, and
    the P = 37 hull in reference mode.  Per tile the probes of the three hulls lie across the surface in the
    shares of assert_shares, and so do the reference mode's (checked beforehand on the CPU oracle's textures of
    the same scenes, which gave at least 0.55 partly submerged, 0.11 dry and 0.12 full over every tile)."""
    w = world
    for t in range(w.T):
        fractions = []
        for p in BODY_PROBES:
            hull, bodies, near = body_case(w, t, p)
            want, f = restate_body(hull, bodies, surface_lookup(w.tex[t], 4))
            got = w.ctx.body_buoyancy(hull, bodies, iterations=4, tile=t)
            assert np.isfinite(got).all()
            np.testing.assert_array_equal(got, want, err_msg=f"tile {t}, P = {p}")
            fractions.append(f.ravel())
            if p == 37:
                want, fr = restate_body(hull, near, reference_lookup(w.tex[t].disp[0]))
                got = w.ctx.body_buoyancy(hull, near, iterations=0, mode=oh.QUERY_REFERENCE, tile=t)
                np.testing.assert_array_equal(got, want, err_msg=f"tile {t}, P = {p}, reference mode")
                assert_shares(fr.ravel(), f"tile {t}, reference mode")
        assert_shares(np.concatenate(fractions), f"tile {t}, K = 4")


def test_surface_grid_every_tile(world):
    """ocean_surface_grid(tile = t): GRID_SURFACE and GRID_HEIGHTFIELD are restate_surface over the grid's
    nodes for K in {0, 1, 4, 16}, GRID_VERTICES the domain stage over O.sample_world at lod 0 and 2.25, all
    over tile t's textures."""
    w = world
    nx, ny = GRID[4], GRID[5]
    q = oh.OceanContext.grid_points(*GRID)
    for t in range(w.T):
        want = restate_surface(w.tex[t], q, KS)
        for k in KS:
            got = w.ctx.surface_grid(*GRID, mode=oh.GRID_SURFACE, iterations=k, tile=t)
            np.testing.assert_array_equal(got, want[k].reshape(ny, nx, 8), err_msg=f"tile {t}, K = {k}")
            h = w.ctx.surface_grid(*GRID, mode=oh.GRID_HEIGHTFIELD, iterations=k, tile=t)
            np.testing.assert_array_equal(h, want[k][:, 0].reshape(ny, nx), err_msg=f"heightfield, tile {t}, K = {k}")
        for lod in (0.0, 2.25):
            s = w.sample(t, np.concatenate([q, np.full((len(q), 1), lod, f32)], axis=1))
            got = w.ctx.surface_grid(*GRID, mode=oh.GRID_VERTICES, lod=lod, tile=t).reshape(-1, 8)
            msg = f"vertices, tile {t}, lod = {lod}"
            np.testing.assert_array_equal(got[:, [0, 2]], q + s[:, 0, [0, 2]], err_msg=msg)  # fp32 + fp32
            np.testing.assert_array_equal(got[:, 1], s[:, 0, 1], err_msg=msg)
            np.testing.assert_array_equal(got[:, 3], s[:, 0, 3], err_msg=msg)
            np.testing.assert_array_equal(got[:, 4:7], s[:, 2, :3], err_msg=msg)
            np.testing.assert_array_equal(got[:, 7], np.zeros(len(q), f32), err_msg=msg)


def test_query_velocity_every_tile(vworld):
    """ocean_query_velocity(tile = t) is restate_velocity over tile t's textures and tile t's VEL."""
    w = vworld
    for t in range(w.T):
        q = w.queries(t)
        want = restate_velocity(w.tex[t], w.vel[t], q, KS)
        for k in KS:
            got = w.ctx.query_velocity(q, tile=t, iterations=k)
            np.testing.assert_array_equal(got, want[k], err_msg=f"tile {t}, K = {k}")
        assert np.abs(want[4][:, :3]).max() > 0


def _device(a, dev):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, f32)).to(dev)


def test_forms_agree_on_a_later_tile(world3):
    """Tile 1 of 3: the blocking form is the restatement, and the _device and _async forms of the query, the
    grid and the bodies, and ocean_sample_world_device, equal the blocking form bit for bit."""
    import torch
    w, t = world3, 1
    ctx, vp = w.ctx, ctypes.c_void_p
    dev = torch.device("cuda", ctx.device)
    # the surface query
    q = w.queries(t)[:1000]
    want = ctx.query_surface(q, tile=t)
    np.testing.assert_array_equal(want, restate_surface(w.tex[t], q, (4,))[4])
    rb = ctx.query_surface_async(q, tile=t)
    np.testing.assert_array_equal(rb.data, want)
    rb.release()
    d_q, d_out = _device(q, dev), torch.zeros(len(q) * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert ctx.lib.ocean_query_surface_device(ctx._h, t, oh.QUERY_SURFACE, 4, vp(d_q.data_ptr()), len(q),
                                              vp(d_out.data_ptr())) == oh.OK
    ctx.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().reshape(-1, 8), want)
    # world sampling
    pts = _points(1000, w.n, 77, lod_max=3.0)
    want = ctx.sample_world(pts, tile=t)
    np.testing.assert_array_equal(want, w.sample(t, pts))
    d_p, d_out = _device(pts, dev), torch.zeros(len(pts) * 12, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    assert ctx.lib.ocean_sample_world_device(ctx._h, t, vp(d_p.data_ptr()), len(pts), vp(d_out.data_ptr())) == oh.OK
    ctx.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().reshape(-1, 3, 4), want)
    # the grid, as records and as a height map
    nodes = oh.OceanContext.grid_points(*GRID)
    rec = restate_surface(w.tex[t], nodes, (4,))[4]
    for mode, per, restated in ((oh.GRID_SURFACE, 8, rec.reshape(GRID[5], GRID[4], 8)),
                                (oh.GRID_HEIGHTFIELD, 1, rec[:, 0].reshape(GRID[5], GRID[4]))):
        want = ctx.surface_grid(*GRID, mode=mode, tile=t)
        np.testing.assert_array_equal(want, restated)
        rb = ctx.surface_grid_async(*GRID, mode=mode, tile=t)
        np.testing.assert_array_equal(rb.data, want)
        rb.release()
        count = GRID[4] * GRID[5] * per
        d_out = torch.zeros(count, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        assert ctx.lib.ocean_surface_grid_device(ctx._h, t, mode, 4, 0.0, *GRID, vp(d_out.data_ptr()), count * 4) == oh.OK
        ctx.synchronize()
        np.testing.assert_array_equal(d_out.cpu().numpy().reshape(want.shape), want)
    # the bodies
    hull, bodies, _ = body_case(w, t, 37)
    want = ctx.body_buoyancy(hull, bodies, tile=t)
    np.testing.assert_array_equal(want, restate_body(hull, bodies, surface_lookup(w.tex[t], 4))[0])
    rb = ctx.body_buoyancy_async(hull, bodies, tile=t)
    np.testing.assert_array_equal(rb.data, want)
    rb.release()
    d_h, d_b = _device(hull, dev), _device(bodies, dev)
    d_out = torch.zeros(BODIES * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.body_buoyancy_device(d_h.data_ptr(), len(hull), d_b.data_ptr(), BODIES, d_out.data_ptr(), tile=t)
    ctx.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().reshape(-1, 8), want)


def test_velocity_forms_agree_on_a_later_tile(vworld3):
    """Tile 2 of 3, the last: the blocking velocity query is the restatement, and the _device and _async forms
    equal it bit for bit."""
    import torch
    w, t = vworld3, 2
    ctx = w.ctx
    q = w.queries(t)[:1000]
    want = ctx.query_velocity(q, tile=t)
    np.testing.assert_array_equal(want, restate_velocity(w.tex[t], w.vel[t], q, (4,))[4])
    rb = ctx.query_velocity_async(q, tile=t)
    np.testing.assert_array_equal(rb.data, want)
    rb.release()
    dev = torch.device("cuda", ctx.device)
    d_q, d_out = _device(q, dev), torch.zeros(len(q) * 8, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.query_velocity_device(d_q.data_ptr(), len(q), d_out.data_ptr(), tile=t)
    ctx.synchronize()
    np.testing.assert_array_equal(d_out.cpu().numpy().reshape(-1, 8), want)


def test_tile_range(world3, vworld3):
    """T = 3: tile 3 and tile -1 are OCEAN_E_INVALID_ARG from the five entries and their async forms (of
    ocean_sample_world, which has none, the device form); tile 2 is served."""
    ctx, vctx = world3.ctx, vworld3.ctx
    pts, q = np.zeros((8, 3), f32), np.zeros((8, 2), f32)
    hull, bodies = oh.OceanContext.box_hull(2, 2), np.zeros((8, 10), f32)
    bodies[:, 6], bodies[:, 7:10] = 1.0, 1.0
    g = (0.0, 0.0, 1.0, 1.0, 4, 4)
    calls = [
        lambda t: ctx.sample_world(pts, tile=t),
        lambda t: ctx.query_surface(q, tile=t),
        lambda t: ctx.query_surface_async(q, tile=t),
        lambda t: ctx.surface_grid(*g, tile=t),
        lambda t: ctx.surface_grid_async(*g, tile=t),
        lambda t: ctx.body_buoyancy(hull, bodies, tile=t),
        lambda t: ctx.body_buoyancy_async(hull, bodies, tile=t),
        lambda t: vctx.query_velocity(q, tile=t),
        lambda t: vctx.query_velocity_async(q, tile=t),
    ]
    for i, call in enumerate(calls):
        for t in (3, -1):
            with pytest.raises(oh.OceanError) as e:
                call(t)
            assert e.value.code == oh.E_INVALID_ARG, (i, t)
    import torch
    dev = torch.device("cuda", ctx.device)
    d_p, d_out = _device(pts, dev), torch.zeros(8 * 12, dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    vp = ctypes.c_void_p
    for t, rc in ((3, oh.E_INVALID_ARG), (-1, oh.E_INVALID_ARG), (2, oh.OK)):
        assert ctx.lib.ocean_sample_world_device(ctx._h, t, vp(d_p.data_ptr()), 8, vp(d_out.data_ptr())) == rc, t
    ctx.synchronize()
    assert ctx.sample_world(pts, tile=2).shape == (8, 3, 4)
    assert ctx.query_surface(q, tile=2).shape == (8, 8)
    assert ctx.surface_grid(*g, tile=2).shape == (4, 4, 8)
    assert ctx.body_buoyancy(hull, bodies, tile=2).shape == (8, 8)
    assert vctx.query_velocity(q, tile=2).shape == (8, 8)
    for rb in (ctx.query_surface_async(q, tile=2), ctx.surface_grid_async(*g, tile=2),
               ctx.body_buoyancy_async(hull, bodies, tile=2), vctx.query_velocity_async(q, tile=2)):
        rb.wait()
        rb.release()
