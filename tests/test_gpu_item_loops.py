"""The item loops of the persistent transform kernels (fftq.hip, fft3.hip, fft4k.hip and the operator passes of
fft2.hip) with a capped launch grid.

The host launches min(items, CUs x resident workgroups per CU) workgroups and each walks
`for (item = blockIdx.x; item < items; item += gridDim.x)`.  On a 256-CU part the small shapes of the exact tests
stay at or near that grid, so a workgroup handles one item, at most two, and the code that carries state from one
item to the next hardly runs there: the register rings two steps ahead, the h0k pair and table key read one item
ahead, d0 staged through LDS, the foam prefetch, the XCD regrouping, the live extent of the next item's unit.
OCEAN_MAX_GROUPS=k caps every such grid at k workgroups (a schedule knob: abi_internal.h ocean_options), and then
those loops iterate at the smallest shapes:

  k = 1  one workgroup crosses every unit boundary in order;
  k = 3  the items are not divisible by the cap, so some workgroups stop an iteration earlier than others;
  k = 8  one workgroup per XCD slot: the regrouped orders combine with a long loop.

The one comparison: a context with the cap and a context without it, same scene, noise and other knobs, are
np.array_equal in every texture after the last of three frames (foam carried, so TURB holds the earlier frames).
This is derived, not measured: both contexts run the same instantiations (kernel_name) and an item's arithmetic
does not depend on which workgroup ran it.  One anchor per kernel family compares the k = 1 context with the
oracle at the suite's tolerance, so that two contexts wrong alike cannot pass."""
import functools

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
from test_gpu_parity import TOL, _ctx_with_env, assert_channels, cplx, oracle_threads
from test_gpu_prune import DENSE, FLAT, SPARSE, TIMES, assert_pruned_against_dense

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

CAPS = (1, 3, 8)
SCENE_A = [DENSE, SPARSE, FLAT]  # with two tiles, the units in order: D>S, S>F, F>D
SCENE_B = [DENSE, FLAT, SPARSE]  # D>F, F>S, S>D


def texs(flags):
    t = [oh.TEX_DISP]
    if not flags & oh.F_DISPLACEMENT_ONLY:
        t += [oh.TEX_DERIV, oh.TEX_TURB]
    if flags & oh.F_NORMALS:
        t.append(oh.TEX_NORMAL)
    if flags & oh.F_VELOCITY:
        t.append(oh.TEX_VELOCITY)
    return t


def ctx_pair(cap, env, n, cas, band=None, **kw):
    """(capped, plain, noises): two contexts that differ in OCEAN_MAX_GROUPS alone."""
    a, noise = _ctx_with_env(dict(env, OCEAN_MAX_GROUPS=str(cap)), n, cas, **kw)
    b, _ = _ctx_with_env(dict(env), n, cas, **kw)
    if band:
        a.set_column_band(*band)
        b.set_column_band(*band)
    return a, b, noise


def last_frame(ctx, tiles=1, flags=0):
    """Every texture of every unit after the last of the three frames."""
    for t in TIMES:
        ctx.step(t)
    return {(tex, tile): ctx.read_all(tex, tile) for tile in range(tiles) for tex in texs(flags)}


def assert_same(a, b, what):
    assert a.keys() == b.keys()
    for tex, tile in a:
        assert np.array_equal(a[tex, tile], b[tex, tile]), f"{what}: texture {tex} of tile {tile} differs"


def assert_same_kernels(a, b, rows=None, cols=None):
    """Both contexts ran the same instantiations; rows / cols name the kernel the case is about."""
    for kind, want in ((0, rows), (1, cols)):
        ka, kb = a.kernel_name(kind), b.kernel_name(kind)
        assert ka == kb, (ka, kb)
        assert not want or want in ka, (want, ka)


def assert_oracle(got, n, cas, noise, tile, flags=0):
    """The last frame of one tile against the oracle's, every channel of every cascade within TOL."""
    nplanes = 2 if flags & oh.F_DISPLACEMENT_ONLY else 4
    oc = O.OracleOcean(n, O.scene_params(), cas, noise, nplanes=nplanes)
    for t in TIMES:
        disp, deriv, turb = oc.step(t)
    assert_channels(got[oh.TEX_DISP, tile][..., :3], disp[..., :3], tol=TOL, what="capped vs oracle, DISP")
    if nplanes == 4:
        assert_channels(got[oh.TEX_DERIV, tile], deriv, tol=TOL, what="capped vs oracle, DERIV")
        assert_channels(got[oh.TEX_TURB, tile][..., :1], turb[..., :1], tol=TOL, what="capped vs oracle, TURB")


# ------------------------------------------------------------ three-plane passes (fftq.hip)
@pytest.mark.parametrize("disp_cached", ["0", "1"])
@pytest.mark.parametrize("tile_w", [None, "16"])
@pytest.mark.parametrize("scene", ["A", "B"])
@pytest.mark.parametrize("cap", CAPS)
def test_three_plane_512(cap, scene, tile_w, disp_cached):
    """N = 512, [dense, sparse, flat] or [dense, flat, sparse] x 2 tiles: six units whose order gives all six
    transitions between unit kinds inside a workgroup's loop.  4-column tiles (the default of a small job) and
    16-column ones; DISP nontemporal (768 items on narrow tiles, 768 % 256 == 0: the XCD regrouping is on) and
    default-policy; the pruned and the dense (OCEAN_PRUNE=0) kernels.  The capped pruned and the capped dense
    context both equal their uncapped twin, and the pruned ones equal the uncapped dense one."""
    n, tiles, cas = 512, 2, SCENE_A if scene == "A" else SCENE_B
    env = {"OCEAN_DISP_CACHED": disp_cached}
    if tile_w:
        env["OCEAN_TILE_W"] = tile_w
    on_k, on, _ = ctx_pair(cap, env, n, cas, tiles=tiles)
    off_k, off, _ = ctx_pair(cap, dict(env, OCEAN_PRUNE="0"), n, cas, tiles=tiles)
    dense = last_frame(off, tiles)
    assert_same(last_frame(on_k, tiles), dense, f"pruned, {cap} workgroups vs dense")
    assert_same(last_frame(off_k, tiles), dense, f"dense, {cap} workgroups vs dense")
    assert_same(last_frame(on, tiles), dense, "pruned vs dense")
    assert_pruned_against_dense(on_k, off_k)
    assert_pruned_against_dense(on, off)
    wt = "0" if tile_w else "4"  # the WT template argument: 0 = the size's own width, 16 at N = 512
    dc = "true" if disp_cached == "1" else "false"
    assert_same_kernels(on_k, on, f"k_pass_aq<512, false, {wt},", f"k_pass_bq<512, false, {wt}, {dc}, true>(")
    assert_same_kernels(off_k, off, f"k_pass_aq<512, false, {wt},", f"k_pass_bq<512, false, {wt}, {dc}, false>(")
    for c in (on_k, on, off_k, off):
        c.close()


def test_three_plane_512_vs_oracle():
    """The anchor of the three-plane passes: one workgroup per launch, the second tile against the oracle."""
    n, tiles, cas = 512, 2, SCENE_A
    ctx, noise = _ctx_with_env({"OCEAN_MAX_GROUPS": "1"}, n, cas, tiles=tiles)
    got = last_frame(ctx, tiles)
    assert "true>(" in ctx.kernel_name(0) and "true>(" in ctx.kernel_name(1)
    assert_oracle(got, n, cas, noise[1], 1)
    ctx.close()


@pytest.mark.parametrize("tile_w", [None, "4"])
@pytest.mark.parametrize("cap", [1, 3])
def test_three_plane_1024(cap, tile_w):
    """N = 1024, [sparse, dense]: the pruned kernels on 8-column tiles and on 4-column ones (OCEAN_TILE_W=4),
    NORMAL written in pass BQ's epilogue."""
    n, cas, flags = 1024, [SPARSE, DENSE], oh.F_NORMALS
    env = {"OCEAN_TILE_W": tile_w} if tile_w else {}
    on_k, on, _ = ctx_pair(cap, env, n, cas, flags=flags)
    off, _ = _ctx_with_env(dict(env, OCEAN_PRUNE="0"), n, cas, flags=flags)
    want = last_frame(on, 1, flags)
    assert_same(last_frame(on_k, 1, flags), want, f"pruned, {cap} workgroups vs pruned")
    assert_same(want, last_frame(off, 1, flags), "pruned vs dense")
    assert_pruned_against_dense(on_k, off)
    assert_same_kernels(on_k, on, f"k_pass_aq<1024, false, {4 if tile_w else 0},", f"k_pass_bq<1024, false, {4 if tile_w else 0},")
    for c in (on_k, on, off):
        c.close()


# ------------------------------------------------------------ four-plane passes (fft3.hip)
# (n, flags, environment, column band, row kernel, column kernel), each with two cascades x two tiles
FOUR_PLANE = [
    pytest.param(16, 0, {}, None, "k_pass_a3<16", "k_pass_b3<16", id="16"),
    pytest.param(64, 0, {}, None, "k_pass_a3<64", "k_pass_b3<64", id="64"),
    pytest.param(128, oh.F_NORMALS, {}, None, "k_pass_a3<128", "k_pass_b3<128", id="128-normals"),
    pytest.param(256, 0, {}, None, "k_pass_a3<256", "k_pass_b3<256", id="256"),
    pytest.param(256, 0, {"OCEAN_TILE_W": "4"}, None, "k_pass_a3<256", "k_pass_b3<256, 4, 1, 4>", id="256-w4"),
    pytest.param(256, 0, {"OCEAN_TILE_W": "32"}, None, "k_pass_a3<256", "k_pass_b3<256, 4, 1, 0>", id="256-w32"),
    pytest.param(512, 0, {"OCEAN_Q": "0"}, None, "k_pass_a4<512", "k_pass_b3<512", id="512-q0"),
    pytest.param(512, 0, {"OCEAN_A4": "0"}, None, "k_pass_a3<512", "k_pass_b3<512", id="512-a3"),
    pytest.param(256, oh.F_DISPLACEMENT_ONLY, {}, None, "k_pass_a4<256", "k_pass_b2d<256", id="256-disp"),
    pytest.param(512, oh.F_DISPLACEMENT_ONLY, {}, None, "k_pass_a8<512", "k_pass_b8<512", id="512-disp"),
    pytest.param(512, 0, {"OCEAN_Q": "0"}, (128, 256), "k_pass_a4<512, true", "k_pass_b3<512", id="512-band-q0"),
    pytest.param(512, 0, {"OCEAN_Q": "1"}, (128, 256), "k_pass_aq<512, true", "k_pass_bq<512, true", id="512-band-q1"),
]


@pytest.mark.parametrize("n,flags,env,band,rows,cols", FOUR_PLANE)
@pytest.mark.parametrize("cap", CAPS)
def test_four_plane(cap, n, flags, env, band, rows, cols):
    """The four-plane row and column passes at every size with its own kernel shape, the two-plane passes of
    displacement-only frames (A4 + B2D at 256, A8 + B8 at 512), the per-texel row pass (OCEAN_A4=0), narrow and
    wide tiles at 256, and a column band of half the columns through the BAND instantiations of both files."""
    tiles, cas = 2, O.SCENE_CASCADES[:2]
    a, b, _ = ctx_pair(cap, env, n, cas, band=band, tiles=tiles, flags=flags)
    assert_same(last_frame(a, tiles, flags), last_frame(b, tiles, flags), f"{cap} workgroups vs uncapped")
    assert_same_kernels(a, b, rows, cols)
    a.close()
    b.close()


def test_four_plane_vs_oracle():
    """The anchor of the four-plane passes: N = 256, one workgroup per launch, the second tile against the oracle."""
    n, tiles, cas = 256, 2, O.SCENE_CASCADES[:2]
    ctx, noise = _ctx_with_env({"OCEAN_MAX_GROUPS": "1"}, n, cas, tiles=tiles)
    assert_oracle(last_frame(ctx, tiles), n, cas, noise[1], 1)
    ctx.close()


# ------------------------------------------------------------ operator IFFT (fft2.hip)
@functools.lru_cache(maxsize=None)
def _random_planes(n):
    """Four planes of four units, shared by the operator cases of one size (never written to)."""
    rng = np.random.default_rng(n)
    planes = rng.standard_normal((4, 4, n, n, 2)).astype(np.float32)
    planes.setflags(write=False)
    return planes


def _operator(ctx, planes, mask):
    for p in range(4):
        for u in range(4):
            ctx.write(oh.TEX_PLANE0 + p, planes[p, u], u // 2, u % 2)
    ctx.ifft2d(mask)
    return np.stack([np.stack([ctx.read_all(oh.TEX_PLANE0 + p, tile) for tile in range(2)]) for p in range(4)])


@pytest.mark.parametrize("mask", [0b1111, 0b0101])
@pytest.mark.parametrize("n", [64, 256, 1024])
@pytest.mark.parametrize("cap", CAPS)
def test_operator_ifft(cap, n, mask):
    """ocean_ifft2d over four units: all four planes in one run of unit-planes, and planes 0 and 2 as two runs;
    at N = 1024 the column launch takes XCD-paired 8-column halves.  The planes outside the mask stay as written."""
    planes = _random_planes(n)
    a, b, _ = ctx_pair(cap, {}, n, O.SCENE_CASCADES[:2], tiles=2)
    ga, gb = _operator(a, planes, mask), _operator(b, planes, mask)
    assert np.array_equal(ga, gb), f"{cap} workgroups vs uncapped"
    for p in range(4):
        if not mask >> p & 1:
            assert np.array_equal(ga[p].reshape(planes[p].shape), planes[p]), f"plane {p} outside the mask written"
    assert_same_kernels(a, b, f"k_rows2<{n}", f"k_cols2<{n}")
    a.close()
    b.close()


def test_operator_ifft_vs_oracle():
    """The anchor of the operator: N = 256, one workgroup per launch, against the reference's radix-2 schedule."""
    n = 256
    planes = _random_planes(n)
    ctx, _ = _ctx_with_env({"OCEAN_MAX_GROUPS": "1"}, n, O.SCENE_CASCADES[:2], tiles=2)
    got = _operator(ctx, planes, 0b1111)
    for p in range(4):
        want = O.ifft2d(np.ascontiguousarray(planes[p]))
        assert O.rel_err(cplx(got[p].reshape(want.shape)), cplx(want)) <= TOL, f"plane {p}"
    ctx.close()


@pytest.mark.parametrize("flags", [oh.F_UNFUSED, oh.F_VELOCITY], ids=["unfused", "velocity"])
@pytest.mark.parametrize("cap", CAPS)
def test_operator_in_frames(cap, flags):
    """N = 128: the reference-shaped frame (evolve, the operator over all four planes, fill), and a fused frame
    with the VELOCITY texture, whose two scratch planes go through the operator."""
    n, tiles, cas = 128, 2, O.SCENE_CASCADES[:2]
    a, b, _ = ctx_pair(cap, {}, n, cas, tiles=tiles, flags=flags)
    assert_same(last_frame(a, tiles, flags), last_frame(b, tiles, flags), f"{cap} workgroups vs uncapped")
    assert_same_kernels(a, b)
    a.close()
    b.close()


# ------------------------------------------------------------ four-step columns (fft4k.hip)
@pytest.mark.parametrize("bands", [None, "4"])
@pytest.mark.parametrize("cap", [1, 3])
def test_four_step_2048(cap, bands):
    """N = 2048, two cascades: pass A3 and the four-step column passes C1 + C2 over both units in one launch
    pair, and per (unit, column band) with OCEAN_C4_BANDS=4; NORMAL written in pass C2's epilogue."""
    n, cas, flags = 2048, O.SCENE_CASCADES[:2], oh.F_NORMALS
    a, b, _ = ctx_pair(cap, {"OCEAN_C4_BANDS": bands} if bands else {}, n, cas, flags=flags)
    assert_same(last_frame(a, 1, flags), last_frame(b, 1, flags), f"{cap} workgroups vs uncapped")
    assert_same_kernels(a, b, "k_pass_a3<2048", "k_col4s2<2048")
    a.close()
    b.close()


def test_four_step_2048_vs_oracle():
    """The anchor of the four-step column passes: one cascade at N = 2048, one workgroup per launch."""
    n, cas = 2048, O.SCENE_CASCADES[:1]
    ctx, noise = _ctx_with_env({"OCEAN_MAX_GROUPS": "1"}, n, cas)
    got = last_frame(ctx)
    O.set_threads(oracle_threads())
    try:
        assert_oracle(got, n, cas, noise[0], 0)
    finally:
        O.set_threads(1)
    ctx.close()


def test_four_step_4096():
    """N = 4096, one cascade, three workgroups: pass A3Q and the four-step passes with the three-plane
    intermediate (C4Q)."""
    n, cas = 4096, O.SCENE_CASCADES[:1]
    a, b, _ = ctx_pair(3, {}, n, cas)
    assert_same(last_frame(a), last_frame(b), "3 workgroups vs uncapped")
    assert_same_kernels(a, b, "k_pass_a3q<4096", "k_col4s2<4096")
    a.close()
    b.close()
