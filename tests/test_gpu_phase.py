"""The phase factor exp(i omega t) on the device.

Part 1: sincos_fast (csrc/spectrum_math.h) read out of k_evolve bit for bit against its numpy restatement
(tests/phase_ref.py, itself held to 2 ulp of float64 in tests/test_phase_math.py) for |x| < 2^17, at positive
and negative times; the library sincosf path behind the hand-over against float64 to a measured ulp bound; and
the same function inside k_evolve_velocity.

Part 2: every row pass per wavenumber.  For each unit of each frame the difference to a float64 frame (phase
formed as the reference forms it: the fp32 product omega * t) is transformed back to the spectrum, and each
mirror-row pair (a pass-A item) and each spatial column (a pass-B item) is held to c times the error the oracle
(the reference's radix-2 algorithm in fp32) shows in the same row or column, or its plane-wide rms where that is
larger.  The norm-relative 1e-5 of the other parity tests cannot see one row's fault under a spectrum that falls
by five decades (tests/test_phase_math.py shows one: 41 times the bound here, 1.6e-6 there).

Part 3: the same bound at N = 2048 and 4096, where the column passes are the four-step k_col4s1 / k_col4s2
(csrc/fft4k.hip) and the row pass at 4096 is k_pass_a3q, or k_pass_a3pp under a column parity (csrc/fftq.hip).
The oracle runs threaded there (a second per 4096^2 frame), and the float64 analysis runs in complex128
torch.fft on the device (phase_ref.TorchRef), which test_reference_backends_agree holds to the numpy one: the
numpy transforms of one 4096^2 frame take longer than the frame, its oracle and its readback together.
tests/test_phase_math.py shows what the bound resolves in a four-step transform: one inter-step twiddle 1e-5 rad
off is 5.1 times sqrt(2) x 1.1 there and 2.1e-6 norm-relative.

k_evolve's launch grid is not under OCEAN_MAX_GROUPS (spectrum.hip grid_for: one lane per texel up to 4 M
texels), so the one call made under that knob runs the same grid; it is kept because the issue asks for it."""
import re

import numpy as np
import pytest

import ocean_hip as oh
import oracle as O
import phase_ref as R
from test_gpu_parity import TOL, _ctx_with_env, assert_channels, oracle_threads
from test_gpu_prune import FLAT, SPARSE

pytestmark = [pytest.mark.gpu, pytest.mark.usefixtures("require_gpu")]

f32, f64, u32 = np.float32, np.float64, np.uint32
N_READ, C_READ = 256, 2
PER_CALL = C_READ * N_READ * N_READ  # 131 072 arguments per ocean_evolve

# docs/MEASUREMENTS.md section 21: the library sincosf behind the hand-over measured 1.566 ulp at the worst
# against float64 over library_path_set(); the bound is that figure rounded up to the next whole ulp
LIB_ULP_BOUND = 2.0


# ------------------------------------------------------------------ part 1: the function itself
def _readout_ctx(n=N_READ, ncasc=C_READ, flags=0, env=None):
    """An unfused context whose every texel has H0 = (1, 0, 0, 0): with WAVES = (0, 1, 0, x), evolve_h and
    planes_of (spectrum_math.h) reduce to PLANE1 = (cos, sin) of fp32(x t); every other term is a product with
    an exact zero."""
    ctx, _ = _ctx_with_env(env or {}, n, O.SCENE_CASCADES[:ncasc], flags=flags | oh.F_UNFUSED)
    h0 = np.zeros((n, n, 4), f32)
    h0[..., 0] = 1.0
    for c in range(ncasc):
        ctx.write(oh.TEX_H0, h0, 0, c)
    return ctx


def _upload_args(ctx, x):
    """x: fp32 [C][N][N] -> WAVES = (0, 1, 0, x)."""
    w = np.zeros(x.shape + (4,), f32)
    w[..., 1] = 1.0
    w[..., 3] = x
    for c in range(x.shape[0]):
        ctx.write(oh.TEX_WAVES, w[c], 0, c)


def _device_sincos(ctx, x, t, zeros=True):
    """(sin, cos) of fp32(x t) out of k_evolve for a flat fp32 array x, PER_CALL arguments per ocean_evolve (the
    last call padded with zeros).  zeros: planes 0, 2 and 3 are asserted all zero."""
    pad = (-x.size) % PER_CALL
    xs = np.concatenate([x, np.zeros(pad, f32)]).reshape(-1, C_READ, N_READ, N_READ)
    s, c = np.empty(xs.shape, f32), np.empty(xs.shape, f32)
    for k, chunk in enumerate(xs):
        _upload_args(ctx, chunk)
        ctx.evolve(t)
        p1 = ctx.read_all(oh.TEX_PLANE1)
        c[k], s[k] = p1[..., 0], p1[..., 1]
        if zeros:
            for p in (oh.TEX_PLANE0, oh.TEX_PLANE2, oh.TEX_PLANE3):
                assert not np.any(ctx.read_all(p)), f"plane {p - oh.TEX_PLANE0} not zero (call {k})"
    return s.reshape(-1)[: x.size], c.reshape(-1)[: x.size]


def _assert_bits(got, want, x, what):
    """Equal as uint32 views; only the sign of a zero is compared by value."""
    same = (got.view(u32) == want.view(u32)) | ((got == 0) & (want == 0))
    if not same.all():
        i = np.flatnonzero(~same)
        k = i[0]
        raise AssertionError(f"{what}: {i.size} of {x.size} differ, first at x = {x[k]!r} ({x[k].view(u32):#010x}): "
                             f"device {got[k]!r}, restatement {want[k]!r}")


@pytest.fixture(scope="module")
def fast_args():
    return np.concatenate(list(R.fast_path_sets().values()))


@pytest.mark.parametrize("t", [1.0, -1.0, 3.0])
def test_sincos_fast_bit_exact(fast_args, t):
    """PLANE1 = the restatement bit for bit for every argument of the five sets with |fp32(x t)| < 2^17.  t = 1:
    the product is exact; t = -1: the quadrant logic's branch for negative n on every argument; t = 3: the
    restatement forms the same fp32 product (a third of the arguments then leave the fast path and are not
    compared here).  Subnormal arguments and results included: the library is built with fp32 denormals on."""
    ctx = _readout_ctx()
    arg = fast_args * f32(t)
    fast = np.abs(arg) < f32(R.HANDOVER)
    assert fast.all() if abs(t) == 1.0 else 0.3 < fast.mean() < 0.9
    s, c = _device_sincos(ctx, fast_args, t)
    ws, wc = R.sincos_fast_np(arg[fast])
    _assert_bits(s[fast], ws, fast_args[fast], f"sin, t = {t}")
    _assert_bits(c[fast], wc, fast_args[fast], f"cos, t = {t}")
    ctx.close()


def test_sincos_fast_bit_exact_under_capped_grid(fast_args):
    """One call under OCEAN_MAX_GROUPS=1 (see the module docstring), negative time."""
    ctx = _readout_ctx(env={"OCEAN_MAX_GROUPS": "1"})
    x = fast_args[:: fast_args.size // PER_CALL][:PER_CALL]
    s, c = _device_sincos(ctx, x, -1.0)
    ws, wc = R.sincos_fast_np(-x)
    _assert_bits(s, ws, x, "sin")
    _assert_bits(c, wc, x, "cos")
    ctx.close()


def test_library_path_ulp_and_non_finite():
    """|x| >= 2^17 (2^17 itself, the 4 096 values above it, 2^20 log-uniform up to 3e38, both signs) goes to the
    library sincosf: against float64 sin / cos of the fp32 argument within LIB_ULP_BOUND.  +-inf and NaN give
    NaN in both components."""
    ctx = _readout_ctx()
    x = R.library_path_set()
    odd = np.array([np.inf, -np.inf, np.nan], f32)
    s, c = _device_sincos(ctx, np.concatenate([x, odd]), 1.0, zeros=False)
    assert np.isnan(s[x.size:]).all() and np.isnan(c[x.size:]).all()
    worst = R.worst_ulp(s[: x.size], c[: x.size], x)
    edge = R.worst_ulp(s[:4097], c[:4097], x[:4097])
    print(f"library sincosf path: worst {worst:.3f} ulp over {x.size} arguments ({edge:.3f} just above 2^17)")
    assert worst <= LIB_ULP_BOUND
    ctx.close()


@pytest.mark.parametrize("t", [65536.0, -65536.0])
def test_evolve_velocity_same_function(t):
    """k_evolve_velocity inlines the same function.  N = 16, one cascade, H0 = (1, 0, 0, 0), WAVES = (0, 1, 0, w)
    with the 256 values of w spread over [1, 4): w t is exact and spans [2^16, 2^18), both paths.  VEL's (y, w)
    channels are the operator IFFT of i w (A - B) = (-w sin, w cos); undone in float64 (fft2 of the un-permuted
    field over N^2), each texel is compared with the restatement (library path: float64 sin / cos).
    Tolerance per texel: 8 * 2^-24 * w * log2(N^2), the standard bound for an N^2-point fp32 transform of
    unit-modulus data times 8 for the constant (the moduli w lie within a factor 4 of each other).  A wrong
    quadrant or path is an error of order w, seven decades above it."""
    n = 16
    ctx = _readout_ctx(n, 1, oh.F_VELOCITY)
    w = np.random.default_rng(16).uniform(1.0, 4.0, (1, n, n)).astype(f32)
    w[0, 0, :4] = [1.0, 2.0, np.nextafter(f32(2.0), f32(0)), np.nextafter(f32(4.0), f32(0))]  # the hand-over itself
    _upload_args(ctx, w)
    ctx.step(t)
    vel = ctx.read(oh.TEX_VELOCITY).astype(f64)
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    got = np.fft.fft2((1 - 2 * ((x + y) % 2)) * (vel[..., 1] + 1j * vel[..., 3])) / (n * n)
    arg = w[0] * f32(t)
    fast = np.abs(arg) < f32(R.HANDOVER)
    assert 0.25 < fast.mean() < 0.75
    s, c = R.sincos_fast_np(arg)
    s = np.where(fast, s.astype(f64), np.sin(arg.astype(f64)))
    c = np.where(fast, c.astype(f64), np.cos(arg.astype(f64)))
    want = w[0].astype(f64) * (-s + 1j * c)
    tol = 8 * 2.0 ** -24 * w[0].astype(f64) * np.log2(n * n)
    err = np.abs(got - want)
    print(f"t = {t}: worst error / tolerance {float((err / tol).max()):.3f}")
    assert (err <= tol).all(), f"worst error / tolerance {float((err / tol).max()):.3g}"
    assert not np.any(vel[..., 0]) and not np.any(vel[..., 2])  # the (x, z) plane: products with kx = kz = 0
    ctx.close()


# ------------------------------------------------------------------ part 2: every row pass, per wavenumber
def _white_h0(n):
    """Unit-modulus random phases in .xy, zeros in .zw: a white spectrum, every wavenumber resolved to a few ulp."""
    ph = np.random.default_rng(64).uniform(0, 2 * np.pi, (n, n))
    h0 = np.zeros((n, n, 4), f32)
    h0[..., 0], h0[..., 1] = np.cos(ph), np.sin(ph)
    return h0


D = oh.F_DISPLACEMENT_ONLY
# id -> (N, cascades (None: the full-band scene of phase_ref.full_band_cascade), flags, knobs, uploaded H0,
#        pattern of kernel_name(0), (c rows, c columns))
# c: the worst ratio measured on an MI355X over units, frames and planes (docs/MEASUREMENTS.md section 21) plus
# about 10 %, the rule of PW_CEILING (test_gpu_parity.py); two independent fp32 roundings of the oracle's size
# give sqrt(2).
CASES = {
    "a3-64-four-planes": (64, None, 0, {}, False, r"k_pass_a3<64, 4,", (1.12, 1.20)),
    "a3-64-two-planes": (64, None, D, {}, False, r"k_pass_a3<64, 2,", (1.19, 1.26)),
    "a3-64-uploaded-h0": (64, None, 0, {}, True, r"k_pass_a3<64, 4,", (0.76, 0.80)),
    "a4-256-two-planes": (256, None, D, {}, False, r"k_pass_a4<256, .*, 2>\(", (1.10, 1.10)),
    "a8-512": (512, None, D, {}, False, r"k_pass_a8<512,", (1.03, 0.96)),
    "a4-512-four-planes": (512, None, 0, {"OCEAN_Q": "0"}, False, r"k_pass_a4<512, .*, 4>\(", (1.01, 1.00)),
    "aq-512-dense": (512, [O.SCENE_CASCADES[0]], 0, {}, False, r"k_pass_aq<512, .*false>\(", (1.46, 1.17)),
    "aq-512-pruned": (512, [SPARSE, FLAT], 0, {}, False, r"k_pass_aq<512, .*true>\(", (1.47, 1.49)),
    "aq-1024-dense": (1024, [O.SCENE_CASCADES[0]], 0, {}, False, r"k_pass_aq<1024, .*false>\(", (1.33, 1.03)),
}


@pytest.mark.parametrize("case", list(CASES))
def test_rows_per_wavenumber(case):
    """Per unit, frame, plane and mirror-row pair y: rms over x of |E(y, .)| <= c max(the oracle's, floor), E =
    fft2(s (gpu - ref)) / N^2, and the same per spatial column with the y-only transform.  Three frames (foam
    carried, compared as in every frame test): t = 100, t = -37.5, and t_x at which a third of the live texels
    are past the hand-over at 2^17, so both paths of sincos_fast meet in one wave."""
    n, cas, flags, env, upload, pattern, (c_row, c_col) = CASES[case]
    full_band = cas is None
    cas = cas or [R.full_band_cascade(n)]
    full = not flags & D
    ctx, (noise,) = _ctx_with_env(env, n, cas, flags=flags)
    oc = O.OracleOcean(n, O.scene_params(), cas, noise, nplanes=4 if full else 2)
    if upload:
        oc.h0[0] = _white_h0(n)
        ctx.write(oh.TEX_H0, oc.h0[0])
    h0, waves = ctx.read_all(oh.TEX_H0), ctx.read_all(oh.TEX_WAVES)
    assert np.array_equal(h0, oc.h0) and np.array_equal(waves, oc.waves)  # the library's own, bit-exact
    times = (100.0, -37.5, R.crossing_time(waves[0], h0[0]))
    worst_rows = worst_cols = blind = 0.0
    for t in times:
        ctx.step(t)
        disp, deriv, turb = oc.step(t)
        g_disp, g_deriv = ctx.read_all(oh.TEX_DISP), (ctx.read_all(oh.TEX_DERIV) if full else None)
        if full:
            assert_channels(ctx.read_all(oh.TEX_TURB), turb, tol=TOL, what=f"{case} t={t:g} turb")
        for u in range(len(cas)):
            ref, spec = R.ref_fields(h0[u], waves[u], t, full)
            got = R.out_fields(g_disp[u], g_deriv[u] if full else None)
            own = R.out_fields(disp[u], deriv[u] if full else None)
            rows, cols = R.frame_ratios(got, own, ref)
            worst_rows, worst_cols = max(worst_rows, rows), max(worst_cols, cols)
            blind = max(blind, R.blind_share(spec, own, ref))
    name = ctx.kernel_name(0)
    ctx.close()
    print(f"{case}: t_x = {times[2]:.6g}, worst row ratio {worst_rows:.3f}, worst column ratio {worst_cols:.3f}, "
          f"rows below the floor {blind:.3f}, kernel {name}")
    assert re.search(pattern, name), name
    if full_band:
        assert blind <= 0.5, "more than half of the rows are checked against the floor only"
    assert worst_rows <= c_row, f"row ratio {worst_rows:.3f} > {c_row}"
    assert worst_cols <= c_col, f"column ratio {worst_cols:.3f} > {c_col}"


# ------------------------------------------------------------------ part 3: N = 2048 and 4096, four-step columns
def _worst_dev(a, b):
    """max |a - b| / max |a| of a numpy field and a device field."""
    b = b.cpu().numpy()
    return float(np.abs(a - b).max() / np.abs(a).max())


def test_reference_backends_agree():
    """phase_ref.TorchRef (complex128 torch.fft on the device) against the numpy functions it restates, N = 256,
    the full-band frame at t = 100, the library's frame and the oracle's as the fp32 fields.  Each function on the
    same input, to 1e-12 relative: ref_fields and its spectrum planes (of each field's maximum); every mirror-row
    pair's rms, every column's rms and both floors of row_rms / col_rms on the numpy error fields d = got - ref
    and d = oracle - ref, uploaded as they are; spec_rows.
    The chain end to end cannot meet 1e-12 in float64 and is held to 1e-6: each backend subtracts its own ref,
    two float64 transforms 2^-53 log2(N^2) ~ 2e-15 of the field apart, from fp32 data 2^-24 ~ 6e-8 of the field
    away from either, so the error fields agree to 3e-8 of their own size and a single row's ratio to some tens
    of that."""
    n, t = 256, 100.0
    cas = [R.full_band_cascade(n)]
    ctx, (noise,) = _ctx_with_env({}, n, cas)
    oc = O.OracleOcean(n, O.scene_params(), cas, noise)
    ctx.step(t)
    disp, deriv, _ = oc.step(t)
    g_disp, g_deriv = ctx.read_all(oh.TEX_DISP), ctx.read_all(oh.TEX_DERIV)
    ctx.close()
    be = R.TorchRef()
    ref, spec = R.ref_fields(oc.h0[0], oc.waves[0], t, True)
    tref, tspec = be.ref_fields(oc.h0[0], oc.waves[0], t, True)
    worst = {"ref_fields": max(_worst_dev(a, b) for a, b in zip(ref, tref)),
             "spectrum": max(_worst_dev(a, b) for a, b in zip(spec, tspec)),
             "spec_rows": max(float(np.abs(be.spec_rows(b) / R.spec_rows(a) - 1).max()) for a, b in zip(spec, tspec))}
    got, own = R.out_fields(g_disp[0], g_deriv[0]), R.out_fields(disp[0], deriv[0])
    tgot, town = be.out_fields(g_disp[0], g_deriv[0]), be.out_fields(disp[0], deriv[0])
    assert all(_worst_dev(a, b) == 0.0 for a, b in zip(got + own, tgot + town))  # fp32 to float64: exact
    for name, mine, theirs in (("row_rms", R.row_rms, be.row_rms), ("col_rms", R.col_rms, be.col_rms)):
        per = floor = 0.0
        for f, r in zip(got + own, ref + ref):
            d = f - r
            (a, fa), (b, fb) = mine(d), theirs(be.torch.from_numpy(d).to(be.device))
            assert a.shape == b.shape == ((n // 2 + 1,) if name == "row_rms" else (n,)) and a.min() > 0
            per, floor = max(per, float(np.abs(b / a - 1).max())), max(floor, abs(fb / fa - 1))
        worst[name], worst[name + " floor"] = per, floor
    a = R.frame_ratios(got, own, ref) + (R.blind_share(spec, own, ref),)
    b = R.frame_ratios(tgot, town, tref, be=be) + (R.blind_share(tspec, town, tref, be=be),)
    chain = max(abs(y / x - 1) for x, y in zip(a[:2], b[:2]))
    print("backends, worst relative difference:", {k: f"{v:.2e}" for k, v in worst.items()},
          f"; end to end: numpy {a}, torch {b}, {chain:.2e} apart")
    for k, v in worst.items():
        assert v <= 1e-12, f"{k}: {v:.2e}"
    assert chain <= 1e-6 and a[2] == b[2]


# id -> (N, cascades (None: the full-band scene), flags, knobs, uploaded H0, column parity, column bands, frames,
#        pattern of kernel_name(0), pattern of kernel_name(1), (c rows, c columns))
# c: by the rule above CASES.  Column bands: OCEAN_C4_BANDS, else the plan's own (frame_plan.h c4_bands: two where
# four planes of 4096^2 exceed 256 MiB, one under a parity or with two planes).  One unit each: the kernels are templates on N, so these are the smallest shapes.
# N = 4096 runs two frames, t = 100 and t_x (both paths of sincos_fast in one frame, and the larger phases):
# a third adds the readback and the transforms of another 4 x 4096^2 frame to each case and runs no other code.
# kernel_name(1) is the last kernel of the column call: k_col4s2<N, P, Q>.  k_col4s1<N, Q> is launched before
# it inside the same call (fft4k.hip launch_pass_c4 / launch_pass_c4q: go_c1<N, Q> then go_c2<N, P, Q>), so the
# k_col4s2 instantiation names its k_col4s1; no index of kernel_name reports it on its own.
# What the plan (csrc/frame_plan.h) picks, against the table of the issue that asked for these cases:
#   - N = 2048 has no three-plane frame and no mirror-pair row pass, so an uploaded H0 (h0k not valid) changes no
#     kernel there: c4-2048-uploaded-h0 runs the kernels of c4-2048-four-planes.  It is kept for its input, a white
#     spectrum in which every row and every inter-step twiddle weighs the same.
#   - at N = 4096 with full outputs the plan picks k_pass_a3q with no knob; k_pass_a3pp is the row pass of a
#     column parity (ocean_set_column_parity).  q-4096-a3pp runs two contexts, one per parity, and interleaves
#     their compact columns into one frame: every mirror-row pair is then one k_pass_a3pp item of each.
#   - q-4096-dense-scene runs the kernels of q-4096-a3q on scene cascade 0, whose band ends inside the grid.
LARGE = {
    "c4-2048-four-planes": (2048, None, 0, {}, False, False, 1, 3,
                            r"k_pass_a3<2048, 4,", r"k_col4s2<2048, 4, false>", (1.18, 1.22)),
    "c4-2048-bands-4": (2048, None, 0, {"OCEAN_C4_BANDS": "4"}, False, False, 4, 3,
                        r"k_pass_a3<2048, 4,", r"k_col4s2<2048, 4, false>", (1.18, 1.22)),
    "c4-2048-two-planes": (2048, None, D, {}, False, False, 1, 3,
                           r"k_pass_a3<2048, 2,", r"k_col4s2<2048, 2, false>", (1.15, 1.07)),
    "c4-2048-uploaded-h0": (2048, None, 0, {}, True, False, 1, 3,
                            r"k_pass_a3<2048, 4,", r"k_col4s2<2048, 4, false>", (0.53, 0.58)),
    "q-4096-a3pp": (4096, None, 0, {}, False, True, 1, 2,
                    r"k_pass_a3pp<4096, (true|false)>", r"k_col4s2<4096, 4, true>", (1.38, 1.13)),
    "q-4096-a3q": (4096, None, 0, {}, False, False, 2, 2,
                   r"k_pass_a3q<4096, false>", r"k_col4s2<4096, 4, true>", (1.36, 1.14)),
    "q-4096-dense-scene": (4096, [O.SCENE_CASCADES[0]], 0, {}, False, False, 2, 2,
                           r"k_pass_a3q<4096, false>", r"k_col4s2<4096, 4, true>", (1.35, 1.12)),
    "c4-4096-two-planes": (4096, None, D, {}, False, False, 1, 2,
                           r"k_pass_a3<4096, 2,", r"k_col4s2<4096, 2, false>", (1.10, 1.15)),
}


def _read_whole(ctxs, tex, n):
    """One unit's texture [1][N][N][4]: the context's own, or the compact halves of the two parity contexts
    (column m of parity b holds x = 2 m + b) interleaved."""
    if len(ctxs) == 1:
        return ctxs[0].read_all(tex)
    out = np.empty((1, n, n, 4), f32)
    for b, ctx in enumerate(ctxs):
        out[:, :, b::2] = ctx.read_all(tex)[:, :, : n // 2]
    return out


@pytest.mark.parametrize("case", list(LARGE))
def test_rows_per_wavenumber_large(case):
    """test_rows_per_wavenumber's assertions at N = 2048 (three frames) and 4096 (two: see LARGE), the float64
    frame and the transforms of the error in complex128 torch.fft on the device (phase_ref.TorchRef), the oracle
    threaded.  Also asserted: kernel_name(1), and one column call per band and frame (kernel_stats).
    The oracle alone on the full-band scene, measured on the CPU before any device run: no row below the floor
    at N = 2048 (t = 100, -37.5, t_x = 49 892) nor at N = 4096 (t = 100, t_x = 49 892), four planes or two
    (blind_share 0.000 in all five frames), so the peak at a quarter of Nyquist still fills the rows."""
    n, cas, flags, env, upload, parity, bands, frames, pat_rows, pat_cols, (c_row, c_col) = LARGE[case]
    full_band = cas is None
    cas = cas or [R.full_band_cascade(n)]
    full = not flags & D
    be = R.TorchRef()
    ctxs = []
    O.set_threads(oracle_threads())
    try:
        for b in range(2 if parity else 1):
            ctx, (noise,) = _ctx_with_env(env, n, cas, flags=flags)
            if parity:
                ctx.set_column_parity(b)
            ctx.set_kernel_timing(True)
            ctxs.append(ctx)
        oc = O.OracleOcean(n, O.scene_params(), cas, noise, nplanes=4 if full else 2)
        if upload:
            oc.h0[0] = _white_h0(n)
            ctxs[0].write(oh.TEX_H0, oc.h0[0])
        h0, waves = ctxs[0].read_all(oh.TEX_H0), ctxs[0].read_all(oh.TEX_WAVES)
        assert np.array_equal(h0, oc.h0) and np.array_equal(waves, oc.waves)  # the library's own, bit-exact
        times = (100.0, -37.5, R.crossing_time(waves[0], h0[0]))
        times = times if frames == 3 else (times[0], times[2])
        worst_rows = worst_cols = (0.0, 0, 0)
        blind = 0.0
        for t in times:
            for ctx in ctxs:
                ctx.step(t)
            disp, deriv, turb = oc.step(t)
            g_disp = _read_whole(ctxs, oh.TEX_DISP, n)
            g_deriv = _read_whole(ctxs, oh.TEX_DERIV, n) if full else None
            if full:
                assert_channels(_read_whole(ctxs, oh.TEX_TURB, n), turb, tol=TOL, what=f"{case} t={t:g} turb")
            ref, spec = be.ref_fields(h0[0], waves[0], t, full)
            got = be.out_fields(g_disp[0], g_deriv[0] if full else None)
            own = be.out_fields(disp[0], deriv[0] if full else None)
            rows, cols = R.frame_ratios(got, own, ref, be=be, where=True)
            worst_rows, worst_cols = max(worst_rows, rows), max(worst_cols, cols)
            blind = max(blind, R.blind_share(spec, own, ref, be=be))
            del ref, spec, got, own, disp, deriv, turb, g_disp, g_deriv
        names = [(ctx.kernel_name(0), ctx.kernel_name(1)) for ctx in ctxs]
        calls = [(ctx.kernel_stats(0)[1], ctx.kernel_stats(1)[1]) for ctx in ctxs]
    finally:
        O.set_threads(1)
        for ctx in ctxs:
            ctx.close()
        be.torch.cuda.empty_cache()
    print(f"{case}: t_x = {times[-1]:.6g}, worst row ratio {worst_rows[0]:.3f} (row pair {worst_rows[1]}, plane "
          f"{worst_rows[2]}), worst column ratio {worst_cols[0]:.3f} (column {worst_cols[1]}, plane {worst_cols[2]}), "
          f"rows below the floor {blind:.3f}, kernels {names}, calls {calls}")
    for (rows_name, cols_name), call in zip(names, calls):
        assert re.search(pat_rows, rows_name), rows_name
        assert re.search(pat_cols, cols_name), cols_name
        assert call == (len(times), bands * len(times))
    if full_band:
        assert blind <= 0.5, "more than half of the rows are checked against the floor only"
    assert worst_rows[0] <= c_row, f"row ratio {worst_rows[0]:.3f} > {c_row}"
    assert worst_cols[0] <= c_col, f"column ratio {worst_cols[0]:.3f} > {c_col}"
