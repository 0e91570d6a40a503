"""Shared by tests/test_phase_math.py (CPU) and tests/test_gpu_phase.py (GPU): the numpy restatement of
sincos_fast (csrc/spectrum_math.h), its argument sets, the ulp measure, and the per-wavenumber analysis of a
frame against a float64 frame whose phase is formed the way the reference forms it (the fp32 product omega * t).

The frame analysis has two backends that state the same formulas: float64 numpy (the module's functions), and
complex128 torch.fft on a device (TorchRef), for the sizes at which the numpy transforms cost more than the
frames they judge.  tests/test_gpu_phase.py holds the two to 1e-12 of each other.

Nothing here is collected by pytest (no test_ prefix) and nothing but TorchRef needs a GPU."""
import sys

import numpy as np

import oracle as O

f32, f64 = np.float32, np.float64
HANDOVER = 131072.0  # sincos_fast: |x| < 2^17 on the Cody-Waite path, the library sincosf from there on
K_MAX = 83442        # the multiples k pi/2 (and (k + 1/2) pi/2) below 2^17 that the argument sets visit

# spectrum_math.h sincos_fast, constant for constant
TWO_OVER_PI = f32(0.636619772367581343)
PIO2_1 = f32(1.57079637050628662109375)
PIO2_2 = f32(-4.37113882867379e-08)
PIO2_3 = f32(-1.7151245e-15)
S1, S2, S3 = f32(-1.6666654611e-1), f32(8.3321608736e-3), f32(-1.9515295891e-4)
C1, C2, C3 = f32(4.166664568298827e-2), f32(-1.388731625493765e-3), f32(2.443315711809948e-5)


def fma32(a, b, c):
    """fmaf: a * b + c of fp32 arrays with ONE rounding.  The product of two fp32 values is exact in float64
    (48 bits); TwoSum gives the float64 sum s and its exact error e; where e != 0 the sum is rounded to odd
    (of the two float64 neighbours of the exact value, the one with an odd significand), which makes the
    final rounding to fp32 equal the direct one (53 >= 24 + 2 bits).  Finite inputs only."""
    a, b, c = (np.asarray(v, f32) for v in (a, b, c))
    p = a.astype(f64) * b.astype(f64)
    c = c.astype(f64)
    s = p + c
    bb = s - p
    e = (p - (s - bb)) + (c - bb)
    s, e = np.broadcast_arrays(s, e)
    even = (s.view(np.uint64) & np.uint64(1)) == 0
    fix = (e != 0) & even
    toward = np.where(e > 0, np.inf, -np.inf)
    return np.where(fix, np.nextafter(s, toward), s).astype(f32)


def fma32_naive(a, b, c):
    """The double-rounding form (float64 a * b + c rounded to float64, then to fp32): what fma32 must beat."""
    return (np.asarray(a, f32).astype(f64) * np.asarray(b, f32).astype(f64) + np.asarray(c, f32).astype(f64)).astype(f32)


def sincos_fast_np(x, third=True, q_abs=False, fma=fma32):
    """sincos_fast for |x| < 2^17, operation by operation in fp32: (sin, cos).
    Mutants (the check of the check): third=False drops the third split term, q_abs=True takes the quadrant
    from |n|."""
    x = np.asarray(x, f32)
    n = np.rint(x * TWO_OVER_PI)
    r = fma(-n, PIO2_1, x)
    r = fma(-n, PIO2_2, r)
    if third:
        r = fma(-n, PIO2_3, r)
    r2 = r * r
    sp = fma(fma(fma(S3, r2, S2), r2, S1), r2 * r, r)
    cp = fma(fma(fma(C3, r2, C2), r2, C1), r2 * r2, fma(f32(-0.5), r2, f32(1.0)))
    ni = n.astype(np.int32)
    q = (np.abs(ni) if q_abs else ni) & 3
    odd = (q & 1) != 0
    ss, cc = np.where(odd, cp, sp), np.where(odd, sp, cp)
    return np.where((q & 2) != 0, -ss, ss), np.where(((q + 1) & 2) != 0, -cc, cc)


def ulp_err(got, exact):
    """|got - exact| in units of the fp32 ulp at the correctly rounded fp32 value of `exact` (float64)."""
    exact = np.asarray(exact, f64)
    cr = np.abs(exact.astype(f32)).astype(f64)
    _, ex = np.frexp(cr)  # cr = m 2^ex, 0.5 <= m < 1: ulp = 2^(ex - 24), the subnormal spacing at least
    ulp = np.ldexp(1.0, np.maximum(ex - 24, -149))
    return np.abs(np.asarray(got, f32).astype(f64) - exact) / ulp


def worst_ulp(s, c, x):
    """Worst ulp error of (s, c) against float64 sin / cos of the fp32 argument x."""
    x64 = np.asarray(x, f32).astype(f64)
    return float(max(ulp_err(s, np.sin(x64)).max(), ulp_err(c, np.cos(x64)).max()))


def _neighbours(v):
    v = v.astype(f32)
    return np.concatenate([np.nextafter(v, f32(-np.inf)), v, np.nextafter(v, f32(np.inf))])


def _below(x0, count):
    """The `count` fp32 values just below x0 > 0."""
    return (np.asarray(x0, f32).view(np.uint32) - np.arange(1, count + 1, dtype=np.uint32)).view(f32)


def fast_path_sets(seed=20251121):
    """The argument sets of the |x| < 2^17 path, name -> fp32 array (seeded: both test files see the same)."""
    rng = np.random.default_rng(seed)
    k = np.arange(1, K_MAX + 1, dtype=f64)
    mag = np.exp(rng.uniform(np.log(1e-30), np.log(HANDOVER), 1 << 20))
    sign = np.where(rng.integers(0, 2, 1 << 20) == 0, 1.0, -1.0)
    tiny = np.array([0.0, -0.0, 2.0 ** -149, -2.0 ** -149, 2.0 ** -126 - 2.0 ** -149, -(2.0 ** -126 - 2.0 ** -149)])
    near = _neighbours(k * (np.pi / 2))
    below = _below(HANDOVER, 4096)
    sets = {
        "uniform": rng.uniform(-HANDOVER, HANDOVER, 1 << 20).astype(f32),
        "log-uniform": np.concatenate([(mag * sign).astype(f32), tiny.astype(f32)]),
        "k pi/2": np.concatenate([near, -(k * (np.pi / 2)).astype(f32)]),       # where sin or cos cancels
        "(k+1/2) pi/2": _neighbours((k + 0.5) * (np.pi / 2)),                   # where rint switches quadrant
        "below 2^17": np.concatenate([below, -below]),
    }
    for name, a in sets.items():
        a[np.abs(a) >= f32(HANDOVER)] = np.nextafter(f32(HANDOVER), f32(0))  # (a draw that rounds up to 2^17)
        assert a.dtype == f32 and np.all(np.abs(a) < HANDOVER), name
    return sets


def library_path_set(seed=20251122):
    """|x| >= 2^17: 2^17 itself, the 4 096 values above it, 2^20 log-uniform magnitudes up to 3e38; both signs."""
    rng = np.random.default_rng(seed)
    above = (f32(HANDOVER).view(np.uint32) + np.arange(0, 4097, dtype=np.uint32)).view(f32)
    mag = np.exp(rng.uniform(np.log(HANDOVER), np.log(3e38), 1 << 20)).astype(f32)
    mag = np.maximum(mag, f32(HANDOVER))
    pos = np.concatenate([above, mag])
    return np.concatenate([pos, -pos])


# ------------------------------------------------------------------ frames per wavenumber
def full_band_cascade(n, params=None):
    """A cascade whose band is the whole grid (cutoff_high above the corner wavenumber; cutoff_low 1e-10 as in
    scene cascade 0, not 0: k = 0 inside the band makes 1 / |k| infinite and the frame NaN, in the reference
    too) and whose wavelength puts the JONSWAP peak of `params` (InitialSpectrum.compute:49: omega_p = 22 (g^2 / (U F))^(1/3),
    k_p = omega_p^2 / g) at a quarter of Nyquist, N / 8 texels from the centre: most spectrum rows then carry
    energy far above the transform's rounding floor."""
    p = params or O.scene_params()
    g, u, fetch = p["gravity"], p["wind_speed"], p["fetch"]
    kp = (22.0 * (g * g / (u * fetch)) ** (1.0 / 3.0)) ** 2 / g
    length = 2.0 * np.pi * (n / 8.0) / kp
    return dict(wavelength=float(np.float32(length)), cutoff_low=1e-10, cutoff_high=1e12, swell=0.4, fade=0.1)


def evolve64(h0, waves, t):
    """oracle.ref64.evolve with the phase formed as the reference forms it: the fp32 product omega * t, then
    sin / cos of that fp32 number in float64 (ref64.evolve multiplies in double: 1e-4 rad away at t = 100)."""
    phase = (waves[..., 3].astype(f32) * f32(t)).astype(f64)
    h0, waves = h0.astype(f64), waves.astype(f64)
    e = np.cos(phase) + 1j * np.sin(phase)
    h = (h0[..., 0] + 1j * h0[..., 1]) * e + (h0[..., 2] + 1j * h0[..., 3]) * np.conj(e)
    ih = 1j * h
    kx, ik, kz = waves[..., 0], waves[..., 1], waves[..., 2]
    aux = -h * ik
    return [ih * kx * ik + 1j * (ih * kz * ik), h + 1j * (aux * kx * kz), ih * kx + 1j * (ih * kz),
            aux * kx * kx + 1j * (aux * kz * kz)]


def ref_fields(h0, waves, t, full):
    """One unit's float64 frame from fp32 h0 / wave data [N][N][4], as the complex (or real) fields the planes
    are packed from: (Dx, Dz), Dy alone, and with full outputs (Dyx, Dyz), (Dxx, Dzz).  Also returns the
    spectrum planes P (for the share of rows that carry energy)."""
    spec = evolve64(h0, waves, t)[:4 if full else 2]
    P = [O.ref64.ifft2d(q) for q in spec]
    out = [P[0], P[1].real.copy()]
    if full:
        out += [P[2], P[3]]
    return out, spec


def out_fields(disp, deriv):
    """The same fields from one unit's fp32 DISP [N][N][>=3] and DERIV [N][N][4] (None: displacement only)."""
    d = disp.astype(f64)
    out = [d[..., 0] + 1j * d[..., 2], d[..., 1].copy()]
    if deriv is not None:
        g = deriv.astype(f64)
        out += [g[..., 0] + 1j * g[..., 1], g[..., 2] + 1j * g[..., 3]]
    return out


def _checker(n):
    y, x = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    return 1.0 - 2.0 * ((x + y) % 2)


def row_rms(d):
    """E(k) = fft2(s d) / N^2, s = (-1)^(x+y): the error of a plane per wavenumber, as seen at the output.
    Returns rms over x of |E(y, .)| for the mirror-row pairs y = 0 .. N/2 (rows y and N - y are one pass-A
    item; rows 0 and N/2 are their own mirrors), and the rms over the whole plane."""
    n = d.shape[0]
    pw = (np.abs(np.fft.fft2(_checker(n) * d) / (n * n)) ** 2).sum(axis=1)
    pair = pw + pw[(n - np.arange(n)) % n]
    return np.sqrt(pair[: n // 2 + 1] / (2 * n)), float(np.sqrt(pw.sum() / (n * n)))


def col_rms(d):
    """The y-only transform of s d, per spatial column x: rms over y (a pass-B item owns columns), and the rms
    over the whole plane."""
    n = d.shape[0]
    pw = (np.abs(np.fft.fft(_checker(n) * d, axis=0) / n) ** 2).sum(axis=0)
    return np.sqrt(pw / n), float(np.sqrt(pw.sum() / (n * n)))


def spec_rows(p):
    """rms of a spectrum plane per mirror-row pair y = 0 .. N/2 (|P|^2 summed over the pair)."""
    n = p.shape[0]
    pw = (np.abs(p) ** 2).sum(axis=1)
    return np.sqrt((pw + pw[(n - np.arange(n)) % n])[: n // 2 + 1] / (2 * n))


def worst_ratio(got, oracle, ref, rms=row_rms, where=False):
    """max over rows (or columns) of rms(got - ref) / max(rms(oracle - ref), floor), floor = the oracle's rms
    over the whole plane.  A plane on which the oracle is exact everywhere has no yardstick: the ratio is then
    0 if `got` is exact too, else inf.  where: also the index of the row pair (or column) of the maximum."""
    mine, _ = rms(got - ref)
    own, floor = rms(oracle - ref)
    den = np.maximum(own, floor)
    if floor == 0.0:
        worst, at = (0.0 if not mine.any() else float("inf")), int(np.argmax(mine))
    else:
        worst, at = float((mine / den).max()), int(np.argmax(mine / den))
    return (worst, at) if where else worst


def frame_ratios(got, oracle, ref, be=None, where=False):
    """got / oracle / ref: lists of fields of one unit of one frame.  (worst row ratio, worst column ratio)
    over the planes.  be: the backend whose row_rms / col_rms take the fields (None: numpy, this module).
    where: each as (ratio, index of the row pair or column, plane)."""
    be = be or sys.modules[__name__]
    out = []
    for rms in (be.row_rms, be.col_rms):
        per = [worst_ratio(g, o, r, rms, True) + (p,) for p, (g, o, r) in enumerate(zip(got, oracle, ref))]
        out.append(max(per))
    return tuple(out) if where else (out[0][0], out[1][0])


def blind_share(spec, oracle, ref, be=None):
    """The share of mirror-row pairs whose own spectrum rms (of the float64 planes `spec`, each |P| summed over
    the pair) is below the floor of its plane, worst plane: such rows are checked against the floor only.  The
    first two fields come from plane 0 and plane 1 (Dy + i Dxz); a real field sees the Hermitian part of its
    plane, which is no smaller in rms than half of it, so the plane's own rms is the measure for all four."""
    be = be or sys.modules[__name__]
    worst = 0.0
    for p, (o, r) in enumerate(zip(oracle, ref)):
        rows = be.spec_rows(spec[p])
        _, floor = be.row_rms(o - r)
        worst = max(worst, float((rows < floor).mean()))
    return worst


def crossing_time(waves, h0, share=1.0 / 3.0):
    """t_x: the time at which about `share` of the live texels (h0 != 0, omega > 0) have omega * t >= 2^17, so
    that both paths of sincos_fast meet in one frame."""
    om = waves[..., 3]
    live = om[(om > 0) & (h0[..., :2] != 0).any(axis=-1)]
    return float(f32(HANDOVER / np.quantile(live.astype(f64), 1.0 - share)))


# ------------------------------------------------------------------ the same analysis in complex128 torch.fft
class TorchRef:
    """ref_fields, out_fields, row_rms, col_rms and spec_rows as above, formula for formula, in float64 /
    complex128 torch on `device`: the float64 numpy transforms of a 4096^2 frame cost more than the frame and its
    oracle together.  The phase is evolve64's: the fp32 product omega * t formed in numpy, then float64 sin / cos
    of that fp32 number (on the device).  Fields stay on the device; the per-row and per-column rms come back as
    numpy arrays, so worst_ratio, frame_ratios and blind_share (be=this object) are the functions above."""

    def __init__(self, device="cuda"):
        import torch
        self.torch, self.device = torch, torch.device(device)
        self._s = {}

    def _dev(self, a, dtype):
        return self.torch.from_numpy(np.ascontiguousarray(a)).to(self.device).to(dtype)

    def _checker(self, n):
        if n not in self._s:
            t = self.torch
            i = t.arange(n, device=self.device)
            self._s[n] = 1.0 - 2.0 * ((i[None, :] + i[:, None]) % 2).to(t.float64)
        return self._s[n]

    def evolve64(self, h0, waves, t):
        T = self.torch
        phase = self._dev(waves[..., 3].astype(f32) * f32(t), T.float64)  # the fp32 product, as evolve64 forms it
        h0, waves = self._dev(h0, T.float64), self._dev(waves, T.float64)
        e = T.complex(T.cos(phase), T.sin(phase))
        h = T.complex(h0[..., 0], h0[..., 1]) * e + T.complex(h0[..., 2], h0[..., 3]) * T.conj(e)
        ih = 1j * h
        kx, ik, kz = waves[..., 0], waves[..., 1], waves[..., 2]
        aux = -h * ik
        return [ih * kx * ik + 1j * (ih * kz * ik), h + 1j * (aux * kx * kz), ih * kx + 1j * (ih * kz),
                aux * kx * kx + 1j * (aux * kz * kz)]

    def ref_fields(self, h0, waves, t, full):
        T = self.torch
        n = h0.shape[0]
        spec = self.evolve64(h0, waves, t)[:4 if full else 2]
        P = [T.fft.ifft2(q) * (n * n) * self._checker(n) for q in spec]  # oracle.ref64.ifft2d
        out = [P[0], P[1].real.clone()]
        if full:
            out += [P[2], P[3]]
        return out, spec

    def out_fields(self, disp, deriv):
        T = self.torch
        d = self._dev(disp, T.float64)
        out = [T.complex(d[..., 0], d[..., 2]), d[..., 1].clone()]
        if deriv is not None:
            g = self._dev(deriv, T.float64)
            out += [T.complex(g[..., 0], g[..., 1]), T.complex(g[..., 2], g[..., 3])]
        return out

    def spec_rows(self, p):
        T = self.torch
        n = p.shape[0]
        pw = (p.abs() ** 2).sum(dim=1)
        pair = pw + pw[(n - T.arange(n, device=self.device)) % n]
        return T.sqrt(pair[: n // 2 + 1] / (2 * n)).cpu().numpy()

    def row_rms(self, d):
        T = self.torch
        n = d.shape[0]
        pw = ((T.fft.fft2(self._checker(n) * d) / (n * n)).abs() ** 2).sum(dim=1)
        pair = pw + pw[(n - T.arange(n, device=self.device)) % n]
        return T.sqrt(pair[: n // 2 + 1] / (2 * n)).cpu().numpy(), float(T.sqrt(pw.sum() / (n * n)))

    def col_rms(self, d):
        T = self.torch
        n = d.shape[0]
        pw = ((T.fft.fft(self._checker(n) * d, dim=0) / n).abs() ** 2).sum(dim=0)
        return T.sqrt(pw / n).cpu().numpy(), float(T.sqrt(pw.sum() / (n * n)))
