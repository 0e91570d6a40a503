"""GPU tests of the whitecap emitters (ocean_whitecaps / _device / _async, csrc/whitecaps.hip).  The yardstick is
numpy over entries that are tested themselves: ocean_sample_world over OceanContext.grid_points(...) at the lod
gives the foam and the displacement of every node (tests/test_gpu_sample.py), ocean_query_velocity with no
fixed-point step the velocity (tests/test_gpu_velocity.py), and a boolean mask with np.flatnonzero the order.  The
kernels run the same fp32 operations in the same order, so every comparison is bit for bit, header included.

Thresholds come from the yardstick's own foam values (below the minimum, above the maximum, quantiles of the
positive values, a value that occurs, to pin >=), so a scene's selection is whatever its water gives.  Natural
foam is exactly 0 wherever TURB >= 1, which is most of a calm scene: with the scene's first cascade alone, or its
first two, at N = 64 the oracle on the CPU finds no foam at all at the frames of make_ctx (nor after more or
later frames), so the one-cascade scene is the scene's 34 m cascade, which folds at 64^2, and the two-cascade
velocity scene its 201 m and 34 m cascades.  The oracle's shares of nodes with foam > 0 over the 300 x 230 grid
at make_ctx's frames: 23.7 % (64, the 34 m cascade), 32.1 % (64, 4 cascades), 3.7 % (128, 2 cascades), 32.1 %
(64, the 201 m and 34 m cascades).  Every scene asserts a threshold that selects between 2 % and 98 % of that
grid, and a synthetic TURB (uniform in [-0.5, 1.5]) gives a known share on a velocity context."""
import ctypes

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_grid import grids as grid_grids
from test_gpu_parity import _ctx_with_env
from test_gpu_query import make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32 = np.float32
MAXREC = oh.WHITECAP_MAX_RECORDS
PIECE = 65536  # points per call of a yardstick entry
SENTINEL = f32(-12345.0)
# row grids of 1, 63, 64, 65, 255, 256, 257 and 1025 nodes: the edges of a wave (64) and of a chunk (256)
ROWS = [(-37.0, 21.0, 0.9, 1.1, m, 1) for m in (1, 63, 64, 65, 255, 256, 257)]
ROW_1025 = (-37.0, 21.0, 0.9, 1.1, 1025, 1)
# 69,000 nodes = 270 chunks: more than the scan workgroup has lanes, so every lane of it owns more than one chunk
BIG = (-37.0, 21.0, 1.3, 0.7, 300, 230)


def all_grids(n, cas):
    return grid_grids(n, cas) + ROWS + [ROW_1025, BIG]


def yardstick(ctx, g, lod=0.0, tile=0):
    """The record of every node of the grid, float32[nx * ny][8], from the point entries."""
    q = oh.OceanContext.grid_points(*g)
    rec = np.zeros((len(q), 8), f32)
    for a in range(0, len(q), PIECE):
        p = q[a:a + PIECE]
        s = ctx.sample_world(np.concatenate([p, np.full((len(p), 1), lod, f32)], axis=1), tile)
        rec[a:a + PIECE, 0] = p[:, 0] + s[:, 0, 0]  # fp32 + fp32, as OCEAN_GRID_VERTICES
        rec[a:a + PIECE, 1] = s[:, 0, 1]
        rec[a:a + PIECE, 2] = p[:, 1] + s[:, 0, 2]
        rec[a:a + PIECE, 3] = s[:, 0, 3]
        if ctx.flags & oh.F_VELOCITY:
            rec[a:a + PIECE, 4:7] = ctx.query_velocity(p, tile, iterations=0)[:, 0:3]
    rec[:, 7] = np.arange(len(q), dtype=f32)
    return rec


def expected(rec, threshold, capacity):
    """(header uint32[8], records [W][8]) of ocean.h's definition over the yardstick's records."""
    idx = np.flatnonzero(rec[:, 3] >= f32(threshold))
    w = min(len(idx), capacity)
    return np.array([len(idx), w, len(rec), capacity, 0, 0, 0, 0], np.uint32), rec[idx[:w]]


def thresholds(foam):
    """name -> threshold, from the foam values themselves."""
    lo, hi = foam.min(), foam.max()
    # (above an all-zero foam: the smallest normal number, so that the compare never meets a denormal)
    above = np.nextafter(hi, f32(np.inf)) if hi > 0 else np.finfo(f32).tiny
    th = {"below": float(lo) - 1.0, "above": float(above), "exact-max": float(hi),
          "exact-median": float(np.sort(foam)[len(foam) // 2])}
    pos = foam[foam > 0]
    if len(pos):
        th["q50"] = float(np.quantile(pos, 0.5).astype(f32))
        th["q90"] = float(np.quantile(pos, 0.9).astype(f32))
        th["exact-positive"] = float(pos.min())
    return th


def raw(ctx, g, threshold, capacity, lod=0.0, tile=0):
    """The blocking form's whole buffer, float32[capacity + 1][8]."""
    buf = np.full((capacity + 1, 8), SENTINEL, f32)
    rc = ctx.lib.ocean_whitecaps(ctx._h, tile, lod, threshold, *g, capacity, buf.ctypes.data, buf.nbytes)
    assert rc == oh.OK, ctx.lib.ocean_last_error()
    return buf


def assert_list(buf, rec, threshold, capacity, msg):
    head, want = expected(rec, threshold, capacity)
    np.testing.assert_array_equal(buf[0].view(np.uint32), head, err_msg=f"header, {msg}")
    np.testing.assert_array_equal(buf[1:1 + len(want)], want, err_msg=msg)
    return int(head[0])


def check_grid(ctx, g, lod=0.0, tile=0):
    """Every threshold at a capacity that holds the list (or the largest there is), then truncated lists.
    Returns the shares of selected nodes."""
    rec = yardstick(ctx, g, lod, tile)
    shares = []
    for name, th in thresholds(rec[:, 3]).items():
        t = int((rec[:, 3] >= f32(th)).sum())
        cap = min(max(t, 1), MAXREC)
        msg = f"grid {g}, lod {lod}, tile {tile}, threshold {name} = {th!r}, capacity {cap}"
        full = raw(ctx, g, th, cap, lod, tile)
        assert assert_list(full, rec, th, cap, msg) == t
        shares.append(t / len(rec))
        if name == "below":
            assert t == len(rec)
        if name == "above":
            assert t == 0
        if name.startswith("exact"):
            assert t >= 1  # the node that holds the value is selected: >=, not >
        for small in {min(max(t - 1, 1), MAXREC), 1} - {cap}:  # a truncated list is the head of the full one
            cut = raw(ctx, g, th, small, lod, tile)
            assert_list(cut, rec, th, small, msg + f" cut to {small}")
            np.testing.assert_array_equal(cut[1:1 + small], full[1:1 + small])
    # the Python method: (T, records[W][8])
    th = thresholds(rec[:, 3])["exact-median"]
    total, got = ctx.whitecaps(th, *g, capacity=MAXREC, lod=lod, tile=tile)
    head, want = expected(rec, th, MAXREC)
    assert total == head[0] and got.shape == (head[1], 8) and got.dtype == f32
    np.testing.assert_array_equal(got, want)
    return shares


# (N, cascades of the scene by index, flags, lods)
SCENES = [pytest.param(64, (3,), 0, (0.0,), id="64x1"),
          pytest.param(64, (0, 1, 2, 3), 0, (0.0,), id="64x4"),
          pytest.param(128, (0, 1), oh.F_MIPS, (0.0, 0.5, 2.25, 99.0), id="128x2-mips"),
          pytest.param(64, (2, 3), oh.F_VELOCITY, (0.0,), id="64x2-velocity")]


@pytest.mark.parametrize("n,which,flags,lods", SCENES)
def test_whitecaps_match_the_point_entries(n, which, flags, lods):
    """Every grid of the grid tests, the row grids across the wave and chunk edges and the 270-chunk grid, for every
    threshold and capacity, at every lod of the scene.  At lod 0 every scene's own foam must give a threshold that
    selects between 2 % and 98 % of the 300 x 230 grid (the oracle's figures are in the module's docstring), so
    the ranks, and on the velocity scene the VEL taps, are those of a partial selection of natural water."""
    cas = [O.SCENE_CASCADES[c] for c in which]
    ctx = make_ctx(n, cas, flags)
    for lod in lods:
        for g in all_grids(n, cas):
            shares = check_grid(ctx, g, lod)
            if g == BIG and lod == 0.0:
                assert any(0.02 <= s <= 0.98 for s in shares), shares
    if flags & oh.F_MIPS:  # the levels matter
        rec0, rec2 = yardstick(ctx, BIG, 0.0), yardstick(ctx, BIG, 2.25)
        assert not np.array_equal(rec0[:, 3], rec2[:, 3])
    if flags & oh.F_VELOCITY:  # ... and so does the velocity
        assert yardstick(ctx, BIG)[:, 4:7].any()
    ctx.close()


def synthetic_turb(n, seed=7):
    rng = np.random.default_rng(seed)
    return np.repeat(rng.uniform(-0.5, 1.5, (n, n, 1)).astype(f32), 4, axis=2)


def test_whitecaps_known_share_on_a_synthetic_turb():
    """TURB uniform in [-0.5, 1.5] (seed 7), uploaded after the steps on a one-cascade velocity context: the share
    of nodes with foam > 0 lies in [0.25, 0.95].  The same texture through the oracle's sampler on the CPU gives
    0.872 (130 x 37), 0.901 (101 x 101) and 0.877 (300 x 230): a texel is below 1 with probability 3/4 and a
    bilinear blend of four more often.  The lists carry the velocity of every selected node."""
    n, cas = 64, O.SCENE_CASCADES[:1]
    ctx = make_ctx(n, cas, oh.F_VELOCITY)
    ctx.write(oh.TEX_TURB, synthetic_turb(n))
    for g in ((-813.7, 405.3, 3.83, 11.21, 130, 37), (-500.0, -500.0, 10.0, 10.0, 101, 101), BIG, ROW_1025):
        rec = yardstick(ctx, g)
        share = float((rec[:, 3] > 0).mean())
        shares = check_grid(ctx, g)
        if g != ROW_1025:  # (the three grids the bound was checked on)
            assert 0.25 <= share <= 0.95, (g, share)
            assert sum(0.02 <= s <= 0.98 for s in shares) >= 3, shares
        # the smallest positive threshold selects exactly the nodes with foam
        th = float(rec[rec[:, 3] > 0, 3].min())
        total, got = ctx.whitecaps(th, *g, capacity=MAXREC)
        assert total == int((rec[:, 3] > 0).sum())
        np.testing.assert_array_equal(got[:, 7], np.flatnonzero(rec[:, 3] > 0)[:MAXREC].astype(f32))
        assert got[:, 4:7].any()
    ctx.close()


def device_list(ctx, g, threshold, capacity, lod=0.0, tile=0, extra=2):
    """The device form into a sentinel-filled buffer with `extra` records of slack behind it."""
    import torch
    o = torch.full(((capacity + 1 + extra) * 8,), float(SENTINEL), dtype=torch.float32, device=torch.device("cuda", ctx.device))
    torch.cuda.synchronize()
    ctx.whitecaps_device(o.data_ptr(), threshold, *g, capacity, lod, tile)
    ctx.synchronize()
    return o.cpu().numpy().reshape(-1, 8)


def test_whitecaps_write_nothing_they_do_not_own():
    """Above the maximum T = W = 0 and only the header is written; a truncated list ends at its capacity; a full
    list leaves the records past W alone."""
    n, cas = 64, O.SCENE_CASCADES[:4]
    ctx = make_ctx(n, cas)
    for g in (ROW_1025, BIG):
        rec = yardstick(ctx, g)
        th = thresholds(rec[:, 3])
        buf = device_list(ctx, g, th["above"], 100)
        np.testing.assert_array_equal(buf[0].view(np.uint32), np.uint32([0, 0, len(rec), 100, 0, 0, 0, 0]))
        np.testing.assert_array_equal(buf[1:], np.full((102, 8), SENTINEL))
        t = int((rec[:, 3] >= f32(th["q50"])).sum())
        assert t > 8
        for cap in (t + 5, t - 1, 5):
            buf = device_list(ctx, g, th["q50"], cap)
            assert_list(buf, rec, th["q50"], cap, f"device form, grid {g}, capacity {cap}")
            np.testing.assert_array_equal(buf[1 + min(t, cap):], np.full((cap + 2 - min(t, cap), 8), SENTINEL))
    ctx.close()


@pytest.mark.parametrize("cap", [1, 3])
def test_whitecaps_do_not_depend_on_the_launch_grid(cap):
    """OCEAN_MAX_GROUPS = 1 and 3: one workgroup walks every chunk in order, or three whose shares differ.  The
    whole buffers are bit-equal to the uncapped context's, and both to the yardstick."""
    n, cas = 64, O.SCENE_CASCADES[:4]
    a, _ = _ctx_with_env({"OCEAN_MAX_GROUPS": str(cap)}, n, cas, flags=oh.F_VELOCITY)
    b, _ = _ctx_with_env({}, n, cas, flags=oh.F_VELOCITY)
    for c in (a, b):
        for t in (0.5, 1.0):
            c.step(t)
    for g in (ROW_1025, BIG):
        rec = yardstick(b, g)
        th = thresholds(rec[:, 3])
        for name in ("below", "q50", "q90", "above"):
            t = int((rec[:, 3] >= f32(th[name])).sum())
            for capacity in {min(max(t, 1), MAXREC), max(t // 2, 1)}:
                la, lb = device_list(a, g, th[name], capacity), device_list(b, g, th[name], capacity)
                np.testing.assert_array_equal(la, lb, err_msg=f"{cap} workgroups, grid {g}, {name}, capacity {capacity}")
                assert_list(la, rec, th[name], capacity, f"{cap} workgroups, grid {g}, {name}")
    assert a.kernel_name(2) == b.kernel_name(2)
    a.close()
    b.close()


def test_whitecaps_tiles():
    """A 3-tile context with its own noise per tile: every tile is checked against that tile's own yardstick."""
    n, cas = 64, O.SCENE_CASCADES[:4]
    ctx = make_ctx(n, cas, tiles=3)
    g = (-813.7, 405.3, 3.83, 11.21, 130, 37)
    foams = []
    for tile in range(3):
        check_grid(ctx, g, tile=tile)
        check_grid(ctx, ROW_1025, tile=tile)
        foams.append(yardstick(ctx, g, tile=tile)[:, 3])
    assert not np.array_equal(foams[0], foams[1]) and not np.array_equal(foams[1], foams[2])
    ctx.close()


def test_whitecaps_forms_agree_and_async_snapshots_behind_later_steps():
    """The three forms write the same list.  The async request made after step t1, with two more steps queued right
    behind it, holds the list of t1 (a second context gives it), not that of t3."""
    n, cas = 256, O.SCENE_CASCADES[:3]
    times = (0.25, 0.5, 0.75)
    g, cap = (-500.0, -500.0, 10.0, 10.0, 101, 101), 4096
    ctx, ref = make_ctx(n, cas, oh.F_VELOCITY, times=()), make_ctx(n, cas, oh.F_VELOCITY, times=())
    for c in (ctx, ref):
        c.step(0.0)  # foam from two frames
    ctx.step(times[0])
    ref.step(times[0])
    rec = yardstick(ref, g)
    th = thresholds(rec[:, 3])["q50"]
    slot = oh.PinnedBuffer((cap + 1) * 32)
    rb = ctx.whitecaps_async(th, *g, capacity=cap, buf=slot)
    assert "k_whitecap_emit" in ctx.kernel_name(2)  # the last of the three launches
    ctx.step(times[1])
    ctx.step(times[2])
    rb.wait()
    assert rb.done()
    total, got = rb.whitecaps()
    head, want = expected(rec, th, cap)
    assert 0 < total == head[0] <= cap
    np.testing.assert_array_equal(rb.view()[0].view(np.uint32), head)
    np.testing.assert_array_equal(got, want)
    rb.release()
    slot.release()
    # now frame t3: another list, and the three forms agree on it
    later_total, later = ctx.whitecaps(th, *g, capacity=cap)
    assert not (later_total == total and np.array_equal(later, got))
    host = raw(ctx, g, th, cap)
    dev = device_list(ctx, g, th, cap, extra=0)
    rb = ctx.whitecaps_async(th, *g, capacity=cap)
    landed = rb.data
    rb.release()
    w = later_total + 1
    np.testing.assert_array_equal(host[:w], dev[:w])
    np.testing.assert_array_equal(host[:w], landed[:w])
    np.testing.assert_array_equal(host[1:w], later)
    assert_list(host, yardstick(ctx, g), th, cap, "frame t3")
    ctx.close()
    ref.close()


def c_call(ctx, form, out, capacity=7, tile=0, nbytes=None):
    args = (ctx._h, tile, 0.0, 0.5, 0.0, 0.0, 1.0, 1.0, 4, 4, capacity, ctypes.c_void_p(out),
            ctypes.c_size_t((capacity + 1) * 32 if nbytes is None else nbytes))
    if form == "host":
        return ctx.lib.ocean_whitecaps(*args), None
    if form == "device":
        return ctx.lib.ocean_whitecaps_device(*args), None
    req = ctypes.c_void_p(0x1234)
    return ctx.lib.ocean_whitecaps_async(*args, ctypes.byref(req)), req.value


def test_whitecaps_contexts_and_errors():
    import torch
    host = np.zeros((8, 8), f32)
    pinned = oh.PinnedBuffer(8 * 32)
    devbuf = torch.zeros(64 + 4, dtype=torch.float32, device=torch.device("cuda", 0))
    torch.cuda.synchronize()
    outs = lambda c: {"host": host.ctypes.data, "async": pinned.ptr.value, "device": devbuf.data_ptr()}  # noqa: E731
    # OCEAN_E_STATE before ocean_init_spectrum, after the argument checks
    ctx = oh.OceanContext(64, 2, 1)
    for form, out in outs(ctx).items():
        assert c_call(ctx, form, out) == (oh.E_STATE, None), form
        assert c_call(ctx, form, out, capacity=0) == (oh.E_INVALID_ARG, None), form
    with pytest.raises(oh.OceanError) as e:
        ctx.whitecaps(0.5, 0.0, 0.0, 1.0, 1.0, 4, 4)
    assert e.value.code == oh.E_STATE
    with pytest.raises(oh.OceanError) as e:
        ctx.whitecaps_async(0.5, 0.0, 0.0, 1.0, 1.0, 4, 4)
    assert e.value.code == oh.E_STATE
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    ctx.step(1.0)
    # what needs the context: the tile; and the device pointer's alignment is refused, not faulted on
    dev = outs(ctx)
    for form, out in dev.items():
        for tile in (1, -1):
            assert c_call(ctx, form, out, tile=tile) == (oh.E_INVALID_ARG, None), (form, tile)
        assert c_call(ctx, form, out, nbytes=7 * 32) == (oh.E_INVALID_ARG, None), form
        rc, req = c_call(ctx, form, out)
        assert rc == oh.OK and (req is not None) == (form == "async"), form
        if req is not None:
            assert ctx.lib.ocean_readback_wait(ctypes.c_void_p(req)) == oh.OK
            ctx.lib.ocean_readback_release(ctypes.c_void_p(req))
    for off in (4, 8, 12):
        assert c_call(ctx, "device", dev["device"] + off) == (oh.E_INVALID_ARG, None)
    for kw in (dict(capacity=0), dict(capacity=MAXREC + 1), dict(lod=-1.0), dict(tile=1)):
        for method in (ctx.whitecaps, ctx.whitecaps_async):
            with pytest.raises(oh.OceanError) as e:
                method(0.5, 0.0, 0.0, 1.0, 1.0, 4, 4, **kw)
            assert e.value.code == oh.E_INVALID_ARG, kw
    ctx.synchronize()
    # without OCEAN_F_VELOCITY floats [4..6] are +0: all bits clear
    total, rec = ctx.whitecaps(-1.0, -40.0, 12.5, 1.7, 0.9, 50, 20)
    assert total == 1000 and rec.shape == (1000, 8)
    assert not rec[:, 4:7].view(np.uint32).any()
    np.testing.assert_array_equal(rec[:, 7], np.arange(1000, dtype=f32))
    ctx.close()
    # DISPLACEMENT_ONLY has no TURB: unsupported, before and after ocean_init_spectrum
    d = oh.OceanContext(64, 2, 1, oh.F_DISPLACEMENT_ONLY)
    for form, out in outs(d).items():
        assert c_call(d, form, out) == (oh.E_UNSUPPORTED, None), form
    d.set_params(O.scene_params(), O.SCENE_CASCADES[:2])
    d.generate_noise(5)
    d.init_spectrum()
    d.step(1.0)
    for form, out in outs(d).items():
        assert c_call(d, form, out) == (oh.E_UNSUPPORTED, None), form
        assert c_call(d, form, out, capacity=0) == (oh.E_INVALID_ARG, None), form
    d.close()
    # a column-parity shard holds half the columns: unsupported, as the queries
    par = oh.OceanContext(4096, 1, 1)
    par.set_params(O.scene_params(), O.SCENE_CASCADES[:1])
    par.generate_noise_device(1)
    par.init_spectrum()
    par.set_column_parity(0)
    for form, out in outs(par).items():
        assert c_call(par, form, out) == (oh.E_UNSUPPORTED, None), form
    par.close()
    pinned.release()


def test_whitecaps_leave_the_frames_unchanged():
    """Three frames with whitecap lists taken in between (all three forms) and three frames without: every texture
    is bit-equal, foam state included, and the context that never asked launched none of the kernels."""
    n, cas = 128, O.SCENE_CASCADES[:2]
    flags = oh.F_MIPS | oh.F_VELOCITY
    a, b = make_ctx(n, cas, flags, times=()), make_ctx(n, cas, flags, times=())
    for t in (0.25, 0.5, 0.75):
        a.step(t)
        b.step(t)
        a.whitecaps(0.01, *BIG, capacity=MAXREC, lod=0.5)
        rb = a.whitecaps_async(0.01, *ROW_1025, capacity=16)
        device_list(a, BIG, 0.0, 300)
        rb.wait()
        rb.release()
    for tex in (oh.TEX_DISP, oh.TEX_DERIV, oh.TEX_TURB, oh.TEX_VELOCITY):
        np.testing.assert_array_equal(a.read_all(tex), b.read_all(tex))
    for level in (1, 3):
        np.testing.assert_array_equal(a.read_mip(oh.TEX_TURB, level), b.read_mip(oh.TEX_TURB, level))
    assert "whitecap" in a.kernel_name(2) and "whitecap" not in b.kernel_name(2)
    a.close()
    b.close()


# The child of test_whitecap_scratch_is_allocated_by_the_first_call: argv = the directories to import from.  It
# prints one JSON line, a list of rounds, each (bytes taken by a stretch without a whitecaps call, by the stretch
# with the context's first one, by the stretch with its second one).
ALLOC_CHILD = r"""
import json, sys
sys.path[:0] = sys.argv[1:]
import torch
import ocean_hip as oh
import oracle as O

g, cap = (-37.0, 21.0, 1.3, 0.7, 300, 230), 1000
out = torch.empty(300 * 230 * 8, dtype=torch.float32, device=torch.device("cuda", 0))
torch.cuda.synchronize()

def make():
    ctx = oh.OceanContext(64, 2, 1, oh.F_VELOCITY)
    ctx.set_params(O.scene_params(), O.SCENE_CASCADES[2:4])
    ctx.generate_noise(5)
    ctx.init_spectrum()
    return ctx

def stretch(ctx, whitecaps):
    ctx.step(0.5)
    rc = ctx.lib.ocean_surface_grid_device(ctx._h, 0, oh.GRID_VERTICES, 0, 0.0, *g, out.data_ptr(), 300 * 230 * 32)
    assert rc == oh.OK
    if whitecaps:
        ctx.whitecaps_device(out.data_ptr(), 0.05, *g, cap)
    ctx.step(1.0)
    ctx.synchronize()

def free():
    return torch.cuda.mem_get_info(0)[0]

first = make()
stretch(first, True)  # every code object is loaded from here on
rounds = []
for _ in range(3):
    ctx = make()
    stretch(ctx, False)
    f0 = free()
    stretch(ctx, False)
    f1 = free()
    stretch(ctx, True)
    f2 = free()
    stretch(ctx, True)
    f3 = free()
    ctx.close()
    rounds.append((f0 - f1, f1 - f2, f2 - f3))
first.close()
print(json.dumps(rounds))
"""


def test_whitecap_scratch_is_allocated_by_the_first_call(tmp_path):
    """A context that never calls the entry allocates no scratch, and nothing is allocated per call after the
    first.  Observed as the device's free memory (hipMemGetInfo) in a fresh process, whose first context has
    loaded every code object before anything is measured: around a stretch of steps and a vertex grid without a
    whitecaps call a context takes nothing; around the same stretch with its first call (the device form: no
    staging) it takes the scratch, 576 KiB, rounded up by the allocator to at most 2 MiB more; around the stretch
    with its second call nothing again.  Free memory belongs to the whole device, so another tenant can move it
    under a round: three fresh contexts are measured and one undisturbed round is asked for.  A scratch allocated
    in ocean_create, or once per call, shows in none."""
    import json
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    # the HSA runtime carves allocations under 2 MiB out of blocks it keeps, which free memory does not show: the
    # child runs with that fragment allocator off, so that every hipMalloc is a driver allocation of its own
    env = dict(os.environ, HSA_DISABLE_FRAGMENT_ALLOCATOR="1")
    r = subprocess.run([sys.executable, "-c", ALLOC_CHILD, os.path.join(root, "ocean-simulation_amd"),
                        os.path.join(root, "oracle")], capture_output=True, text=True, timeout=120, cwd=str(tmp_path),
                       env=env)
    assert r.returncode == 0, r.stderr
    rounds = json.loads(r.stdout.strip().splitlines()[-1])
    scratch = (oh.GRID_MAX_NODES // 64) * 8 + (oh.GRID_MAX_NODES // 256) * 4
    print("free-memory deltas per round (idle, first call, second call):", rounds, "scratch:", scratch)
    assert scratch == 576 << 10
    clean = [idle == 0 and scratch <= first <= scratch + (2 << 20) and second == 0 for idle, first, second in rounds]
    assert any(clean), rounds
