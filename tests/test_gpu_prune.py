"""Band-limited cascades: passes AQ / BQ skip the rows of a unit's spectrum that are
all zero.  Pass AQ runs the live mirror-pair items only and pass BQ takes the stage-0 inputs of dead rows
as zeros without loading them, so the outputs are those of the dense schedule (OCEAN_PRUNE=0) value for
value; only the sign of a zero may differ, which np.array_equal does not see.

Every case runs at N = 512 unless it says otherwise, with at most 6 units and 3 frames (foam carried)."""
import math

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_parity import TOL, _ctx_with_env, assert_channels, make_ctx

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

TIMES = (0.0, 0.5, 250.0)
TEXS = (oh.TEX_DISP, oh.TEX_DERIV, oh.TEX_TURB)
DENSE = O.SCENE_CASCADES[0]
SPARSE = O.SCENE_CASCADES[3]  # L = 34, cutoff_high = 10
FLAT = dict(DENSE, cutoff_low=1e6)


def live_extent(h0):
    """The largest |y - N/2| over the rows of h0 [N][N][4] whose h0(k) holds a non-zero texel, -1 if none."""
    n = h0.shape[0]
    rows = np.flatnonzero((h0[..., :2] != 0).any(axis=(1, 2)))
    return int(np.abs(rows - n // 2).max()) if rows.size else -1


def frames(ctx, tiles=1, times=TIMES):
    """DISP, DERIV and TURB of every unit after every frame."""
    out = []
    for t in times:
        ctx.step(t)
        out.append([ctx.read_all(tex, tile) for tile in range(tiles) for tex in TEXS])
    return out


def assert_frames_equal(a, b, what):
    for f, (fa, fb) in enumerate(zip(a, b)):
        for k, (xa, xb) in enumerate(zip(fa, fb)):
            assert np.array_equal(xa, xb), f"{what}: frame {f}, tile {k // 3}, texture {TEXS[k % 3]} differs"


def assert_pruned_against_dense(on, off):
    """The comparison is the pruned kernels against the dense ones: both passes of `on` ran their PRUNE
    instantiations (the last template argument), both passes of `off` the dense ones."""
    for kind in (0, 1):
        a, b = on.kernel_name(kind), off.kernel_name(kind)
        assert "true>(" in a and "false>(" in b, (a, b)


def on_and_off(n, cas, **kw):
    on, noise = make_ctx(n, cas, **kw)
    off, _ = _ctx_with_env({"OCEAN_PRUNE": "0"}, n, cas, **kw)
    return on, off, noise


@pytest.mark.parametrize("tile_w", [None, "16"])
def test_on_equals_off(tile_w, monkeypatch):
    """[dense, sparse, flat]: the default context equals an OCEAN_PRUNE=0 context of the same process, and
    the sparse and dense units match the oracle.  Small jobs at N = 512 take 4-column tiles; OCEAN_TILE_W=16
    runs the wide-tile kernels on the same scene."""
    if tile_w:
        monkeypatch.setenv("OCEAN_TILE_W", tile_w)
    n, cas = 512, [DENSE, SPARSE, FLAT]
    on, off, noise = on_and_off(n, cas)
    assert [live_extent(on.read(oh.TEX_H0, 0, c)) for c in range(3)] == [n // 2, 54, -1]
    oc = O.OracleOcean(n, O.scene_params(), cas, noise[0])
    fa, fb = frames(on), frames(off)
    assert_frames_equal(fa, fb, "prune on vs off")
    assert_pruned_against_dense(on, off)
    for t in TIMES:
        disp, deriv, turb = oc.step(t)
    for got, ref in zip(fa[-1], (disp[..., :3], deriv, turb[..., :1])):
        assert_channels(got[:2, ..., :ref.shape[-1]], ref[:2], tol=TOL, what="pruned vs oracle")
    on.close()
    off.close()


def _edge_ctxs(n, m, tile_w=None):
    """One cascade with L = 100 whose band ends at (m + 0.5) dk: rows |y - N/2| <= m are live.  m = 0: no
    texel but k = 0 lies within 0.5 dk, so the band ends at 1.5 dk and the noise of the rows N/2 +- 1 is
    zero, which leaves the centre row alone live.  A flat second cascade shares the chunk: the library runs
    the pruned kernels only for a chunk with at least an eighth of its items dead, and with the flat unit
    beside it every extent, 255 and the dense 256 included, goes through them.  tile_w: OCEAN_TILE_W of both."""
    dk = 2 * math.pi / 100.0
    cas = [dict(wavelength=100.0, cutoff_low=1e-6, cutoff_high=(max(m, 1) + 0.5) * dk, swell=0.3, fade=0.1), FLAT]
    noise = O.generate_noise(n, 20251121)
    if m == 0:
        noise[n // 2 - 1] = 0
        noise[n // 2 + 1] = 0
    ctxs = []
    for env in ({}, {"OCEAN_PRUNE": "0"}):
        c, _ = _ctx_with_env(dict(env, OCEAN_TILE_W=tile_w) if tile_w else env, n, cas)
        c.set_noise(0, noise)
        c.init_spectrum()
        ctxs.append(c)
    return ctxs


EDGES = [(512, 0), (512, 1), (512, 31), (512, 32), (512, 33), (512, 255), (512, 256), (1024, 63), (1024, 64), (1024, 65)]
# two units are a small job, so N = 512 takes 4-column tiles and N = 1024 its 8-column ones: the row groups again
# on the wide tiles of 512 (CT::in_dy of a 16-column tile) and on the narrow ones of 1024
EDGES_W = [(512, 31, "16"), (512, 32, "16"), (512, 33, "16"), (1024, 63, "4"), (1024, 64, "4"), (1024, 65, "4")]


@pytest.mark.parametrize("n,m,tile_w", [pytest.param(n, m, None, id=f"{n}-{m}") for n, m in EDGES] +
                         [pytest.param(n, m, w, id=f"{n}-{m}-w{w}") for n, m, w in EDGES_W])
def test_extent_on_every_edge(n, m, tile_w):
    """Live extents on either side of pass BQ's stage-0 row groups (32 rows at N = 512, 64 at 1024), the
    centre row alone, every row but row 0 (255) and the dense unit (256)."""
    on, off = _edge_ctxs(n, m, tile_w)
    assert [live_extent(on.read(oh.TEX_H0, 0, c)) for c in range(2)] == [m, -1]
    assert_frames_equal(frames(on), frames(off), f"extent {m}")
    assert_pruned_against_dense(on, off)
    on.close()
    off.close()


@pytest.mark.parametrize("first,then", [([DENSE], [SPARSE]), ([SPARSE], [DENSE]), ([DENSE], [FLAT]),
                                        ([DENSE, FLAT], [FLAT, DENSE]), ([DENSE, SPARSE], [FLAT, FLAT])])
def test_stale_intermediate(first, then):
    """A context re-parameterised from one scene to the other equals a fresh context: pass BQ takes nothing
    from the rows the earlier scene left in the intermediate and the side arrays.  A unit that turns flat has
    no live row at all, and an all-flat chunk launches no pass AQ: everything in its region is stale."""
    n = 512
    ctx, _ = make_ctx(n, first)
    ctx.step(0.25)
    ctx.set_params(O.scene_params(), then)
    ctx.init_spectrum()
    ctx.reset_foam()
    fresh, _ = make_ctx(n, then)
    assert_frames_equal(frames(ctx), frames(fresh), "re-parameterised vs fresh")
    ctx.close()
    fresh.close()


@pytest.mark.parametrize("cas,tiles,chunk_mib", [([DENSE, SPARSE], 3, "12"), ([DENSE, SPARSE], 3, "6"),
                                                 ([DENSE, SPARSE], 3, "8"), ([DENSE, FLAT], 3, "8"),
                                                 ([DENSE, FLAT, SPARSE], 2, "12")])
def test_chunks_of_mixed_units(cas, tiles, chunk_mib):
    """Six units in chunks, each equal to the unchunked context.  The intermediate holds the larger of a
    four-plane and a three-plane chunk, so at 12 MiB it has two unit slots and at 8 MiB one, which every chunk
    reuses (at 6 MiB a four-plane chunk is the whole frame, and every unit keeps its own slot).  At 8 MiB dense
    and sparse, or dense and flat, units alternate in the one slot and its side arrays; with three cascades and
    two slots the chunks are (dense, flat), (sparse, dense), (flat, sparse), so each slot sees all three.  A
    flat unit then sits over the rows a live one left there, which a fresh allocation's zeros cannot hide."""
    n = 512
    whole, _ = _ctx_with_env({"OCEAN_CHUNK_MIB": "0"}, n, cas, tiles=tiles)
    parts, _ = _ctx_with_env({"OCEAN_CHUNK_MIB": chunk_mib}, n, cas, tiles=tiles)
    assert_frames_equal(frames(parts, tiles), frames(whole, tiles), f"chunks of {chunk_mib} MiB vs whole")
    whole.close()
    parts.close()


def test_uploaded_h0_is_not_pruned():
    """An uploaded H0 with energy in rows outside the cascade's band: the frame runs the four-plane passes
    on all of it and matches an unfused context given the same H0."""
    n, cas = 512, [SPARSE]
    a, _ = make_ctx(n, cas)
    b, _ = make_ctx(n, cas, flags=oh.F_UNFUSED)
    a.step(0.0)  # a pruned frame first: its extents must not outlive the upload
    h0 = a.read(oh.TEX_H0)
    assert live_extent(h0) == 54
    rng = np.random.default_rng(7)
    for y in (3, 100, 400, 509):  # rows and mirror rows outside the band, .zw = conj of the mirror texel
        h0[y, :, :2] = rng.standard_normal((n, 2)).astype(np.float32) * 1e-3
    mirror = np.roll(h0[::-1, ::-1, :2], (1, 1), axis=(0, 1))
    h0[..., 2] = mirror[..., 0]
    h0[..., 3] = -mirror[..., 1]
    assert live_extent(h0) == 253
    a.write(oh.TEX_H0, h0)
    b.write(oh.TEX_H0, h0)
    a.reset_foam()
    for t in TIMES:
        a.step(t)
        b.step(t)
    for tex in TEXS:
        ref = b.read_all(tex)
        assert_channels(a.read_all(tex)[..., :1 if tex == oh.TEX_TURB else 4], ref[..., :1 if tex == oh.TEX_TURB else 4],
                        tol=TOL, what=f"uploaded H0, texture {tex}")
    a.close()
    b.close()


def test_order_and_tiles_at_1024():
    """[sparse, dense] x 2 tiles at N = 1024: the unit -> cascade mapping of the item table."""
    n, cas, tiles = 1024, [SPARSE, DENSE], 2
    on, off, _ = on_and_off(n, cas, tiles=tiles)
    assert [live_extent(on.read(oh.TEX_H0, 1, c)) for c in range(2)] == [54, n // 2]
    assert_frames_equal(frames(on, tiles), frames(off, tiles), "prune on vs off")
    assert_pruned_against_dense(on, off)
    on.close()
    off.close()
