"""The atmosphere of include/ocean/ocean.h ("The atmosphere") in numpy, statement by statement and generic over the
dtype: in float32 it reproduces the stated order of operations, the multiscatter table's butterfly included (numpy's
fp32 +, -, *, / and sqrt round once, as the kernels'; exp, sin, cos, pow and the inverse functions are numpy's, not the
device library's); in float64, from the same fp32 inputs, it is the analysis that measures what fp32 costs.  Tables
are [H][W][4]."""
import numpy as np

f32 = np.float32
PI32 = f32(3.14159265)            # the compute shaders' PI
CAM_PI32 = f32(3.14159265358979)  # the camera's pi
TINY32 = f32(1.175494351e-38)
SUN_KEYS = (0.01, 0.14, 0.28, 0.36, 0.57, 0.75, 0.86, 0.99)
QUIET = dict(over="ignore", invalid="ignore", divide="ignore")


class Params:
    """ocean.h's names over the float32[32] array, in dtype t."""

    def __init__(self, params, t):
        p = np.asarray(params, f32).astype(t)
        self.t = t
        self.Rp, self.Ra = p[0], p[1]
        self.RS, self.RA, self.HR = p[2:5], p[5:8], p[8]
        self.MS, self.MA, self.HM, self.g = p[9:12], p[12:15], p[15], p[16]
        self.OS, self.OA, self.GA, self.SZ = p[17:20], p[20:23], p[23:26], p[26]
        self.RE, self.ME, self.OE = self.RS + self.RA, self.MS + self.MA, self.OS + self.OA
        self.pi = t(PI32)

    def densities(self, h):
        t = self.t
        dr = np.exp((-h) / self.HR)
        dm = np.exp((-h) / self.HM)
        dz = np.maximum(t(0), t(1) - (h - t(25000)) / t(15000))
        return dr, dm, dz

    @staticmethod
    def mix(r, m, o, d):
        """(r_c * dr + m_c * dm) + o_c * dz, with a trailing channel axis."""
        dr, dm, dz = (x[..., None] for x in d)
        return (r * dr + m * dm) + o * dz

    def texel_radius_mu(self, W, H):
        """rad [1][W], mu [H][1] of a W x H table."""
        t = self.t
        u = (np.arange(W).astype(t) + t(0.5)) / t(W)
        v = (np.arange(H).astype(t) + t(0.5)) / t(H)
        return (u * (self.Ra - self.Rp) + self.Rp)[None, :], (t(-1) + v * t(2))[:, None]


def clamp01(a, t):
    return np.minimum(np.maximum(a, t(0)), t(1))


def _taps(c, n, t):
    x = np.minimum(np.maximum(clamp01(c, t) * t(n) - t(0.5), t(0)), t(n - 1))
    x0 = x.astype(np.int64)
    return x0, np.minimum(x0 + 1, n - 1), (x - x0.astype(t))[..., None]


def lut_read(L, u, v, t):
    """READ(L, u, v): u, v of one shape -> [...][4] (NaN coordinates become 0, as fmaxf makes them)."""
    L = np.asarray(L).astype(t)
    H, W = L.shape[:2]
    u, v = np.broadcast_arrays(np.nan_to_num(np.asarray(u, t), nan=0.0), np.nan_to_num(np.asarray(v, t), nan=0.0))
    x0, x1, fx = _taps(u, W, t)
    y0, y1, fy = _taps(v, H, t)
    lo = L[y0, x0] + fx * (L[y0, x1] - L[y0, x0])
    hi = L[y1, x0] + fx * (L[y1, x1] - L[y1, x0])
    out = lo + fy * (hi - lo)
    assert out.dtype == t
    return out


def lut_at(P, L, sr, cos_a):
    t = P.t
    return lut_read(L, (sr - P.Rp) / (P.Ra - P.Rp), t(0.5) + t(0.5) * cos_a, t)[..., :3]


def transmittance_at(P, rad, mu):
    """The transmittance march from the distance rad to the centre along the cosine mu (arrays of one shape): [...][3]."""
    t = P.t
    rad, mu = np.broadcast_arrays(np.asarray(rad, t), np.asarray(mu, t))
    with np.errstate(**QUIET):
        disc = np.maximum(t(0), (rad * rad) * (mu * mu - t(1)) + P.Ra * P.Ra)
        step = np.maximum(t(0), (-rad) * mu + np.sqrt(disc)) / t(500)
        E = np.zeros(rad.shape + (3,), t)
        two = (t(2) * rad) * mu
        for i in range(500):
            d = (t(i) + t(0.5)) * step
            sr = np.sqrt((d * d + two * d) + rad * rad)
            E = E + P.mix(P.RE, P.ME, P.OE, P.densities(sr - P.Rp)) * step[..., None]
        out = np.exp(-E)
    assert out.dtype == t and E.dtype == t
    return out


def transmittance(params, W, H, t=f32):
    P = Params(params, t)
    out = np.zeros((H, W, 4), t)
    out[..., :3] = transmittance_at(P, *P.texel_radius_mu(W, H))
    return out


def _march(P, rad, dirs, start, step, T, sun_mu, extra=None):
    """The 32 steps both marches share: (L, F, t_end); ins_c = extra(sr, d, tsun, sca) or the multiscatter's."""
    t = P.t
    dx, dy, dz = dirs
    tr = np.ones(step.shape + (3,), t)
    L, F = np.zeros_like(tr), np.zeros_like(tr)
    cur = step * t(0.5) + start if start is not None else step * t(0.5)
    for _ in range(32):
        px, py, pz = cur * dx, rad + cur * dy, cur * dz
        sr = np.sqrt((px * px + py * py) + pz * pz)
        d = P.densities(sr - P.Rp)
        sca, ext = P.mix(P.RS, P.MS, P.OS, d), P.mix(P.RE, P.ME, P.OE, d)
        tsun = lut_at(P, T, sr, sun_mu)
        ins = extra(sr, d, tsun, sca) if extra else (tsun * sca) * (t(1) / (t(4) * P.pi))
        nt = tr * np.exp((-ext) * step[..., None])
        ti = (tr - nt) / ext
        L = L + ti * ins
        F = F + ti * sca
        cur = cur + step
        tr = nt
    assert L.dtype == t
    return L, F, tr


def butterfly(a):
    """The fixed butterfly over axis -2 of [...][64][3]: fold the upper half onto the lower half until one is left."""
    while a.shape[-2] > 1:
        h = a.shape[-2] // 2
        a = a[..., :h, :] + a[..., h:, :]
    return a[..., 0, :]


def multiscatter(params, T, W, H, t=f32):
    P = Params(params, t)
    rad, mu = P.texel_radius_mu(W, H)
    rad, mu = (np.broadcast_to(a, (H, W))[..., None] for a in (rad, mu))  # [H][W][1] against the 64 lanes
    with np.errstate(**QUIET):
        z = (np.arange(64).astype(t) + t(0.5)) / t(64)
        xy = np.sqrt(t(1) - z * z)
        az = ((z * t(8)) * P.pi) * t(2)
        dx, dy, dz = (np.broadcast_to(a, (H, W, 64)) for a in (np.sin(az) * xy, np.cos(az) * xy, z))
        off = (-rad) * dy
        rc2 = rad * rad - off * off
        p2 = P.Rp * P.Rp
        hit = (rc2 < p2) & (dy < 0)
        end = np.where(hit, off - np.sqrt(np.where(hit, p2 - rc2, t(0))), np.sqrt(P.Ra * P.Ra - rc2) + off)
        step = end / t(32)
        L, F, tr = _march(P, rad, (dx, dy, dz), None, step, T, mu)
        ground = ((tr * lut_at(P, T, np.broadcast_to(rad, (H, W, 64)), mu)) * (P.GA / P.pi)) * mu[..., None]
        L = np.where(hit[..., None], L + ground, L)
        L, F = butterfly(L), butterfly(F)
        out = np.ones((H, W, 4), t)
        out[..., :3] = L / (t(64) - F)
    assert out.dtype == t and L.dtype == t
    return out


def normalise_sun(sun, t=f32):
    """ocean_sky_update's host normalisation, always in fp32 (it is the kernels' input), then cast to t."""
    s = np.asarray(sun, f32)
    ln = np.sqrt((s[0] * s[0] + s[1] * s[1]) + s[2] * s[2])
    return (s / ln).astype(f32).astype(t)


def skyview(params, T, M, sun, W, H, t=f32):
    """(S, ends): the sky-view table for `sun` (any length) and the texels whose ray ends on the planet."""
    P = Params(params, t)
    s = normalise_sun(sun, t)
    with np.errstate(**QUIET):
        lon = (-P.pi + ((np.arange(W).astype(t) + t(0.5)) / (t(W) - t(1))) * (t(2) * P.pi))[None, :]
        v = (t(1) - (np.arange(H).astype(t) + t(0.5)) / (t(H) - t(1)))[:, None]
        rad = P.Rp
        beta = np.arccos(np.sqrt(rad * rad - P.Rp * P.Rp) / rad)
        zha = P.pi - beta
        a = v * t(2) - t(1)
        a = a * a
        lat = np.where(v < t(0.5), (t(1) - a) * zha, zha + a * beta)
        sl, cl = np.sin(lat), np.cos(lat)
        dx, dy, dz = (np.broadcast_to(x, (H, W)) for x in (np.sin(lon) * sl, cl, np.cos(lon) * sl))
        cs = (dx * s[0] + dy * s[1]) + dz * s[2]
        g = P.g
        PR = (t(3) / (t(16) * P.pi)) * (t(1) + cs * cs)
        PM = ((t(3) / (t(8) * P.pi)) * ((t(1) - g * g) * (t(1) + cs * cs))) / \
            ((t(2) + g * g) * np.power(np.abs((t(1) + g * g) - (t(2) * g) * cs), t(1.5)))
        off = (-rad) * dy
        rc2 = rad * rad - off * off
        p2 = P.Rp * P.Rp
        top = np.sqrt(P.Ra * P.Ra - rc2)
        start = np.maximum(t(0), off - top)
        ends = (rc2 < p2) & (dy < 0)
        end = np.where(ends, off - np.sqrt(np.where(ends, p2 - rc2, t(0))), top + off)
        step = (end - start) / t(32)

        def ins(sr, d, tsun, sca):
            dr, dm = d[0][..., None], d[1][..., None]
            x = tsun * (dr * (P.RS * PR[..., None]) + dm * (P.MS * PM[..., None]))
            return x + lut_at(P, M, sr, s[1]) * sca

        L, _, _ = _march(P, np.broadcast_to(rad, (H, W)), (dx, dy, dz), start, step, T, s[1], ins)
        out = np.ones((H, W, 4), t)
        out[..., :3] = np.power(np.abs(L), t(f32(1) / f32(2.2)))
    assert out.dtype == t and L.dtype == t
    return out, ends


def sun_color(column, sun, t=f32):
    """ocean_sun_color over column 0 of the transmittance table, [H][>=3]."""
    col = np.asarray(column).astype(t)[:, :3]
    H = col.shape[0]
    keys = []
    for tk in SUN_KEYS:
        y = min(max(t(f32(tk)) * t(H) - t(0.5), t(0)), t(H - 1))
        y0 = int(y)
        y1 = min(y0 + 1, H - 1)
        keys.append((col[y0] + (y - t(y0)) * (col[y1] - col[y0])) * t(2.5))
    tk = [t(f32(k)) for k in SUN_KEYS]
    e = (normalise_sun(sun, t)[1] + t(1)) * t(0.5)
    if e <= tk[0]:
        return keys[0]
    if e >= tk[7]:
        return keys[7]
    k = max(i for i in range(7) if tk[i] <= e)
    f = (e - tk[k]) / (tk[k + 1] - tk[k])
    out = keys[k] + f * (keys[k + 1] - keys[k])
    assert out.dtype == t
    return out


# ---------------------------------------------------------------------------- the camera's sky mode
def sky_lookup(S, r, t=f32):
    """SKY(r): r [M][3] of any length -> [M][3]."""
    r = np.asarray(r).astype(t)
    pi = t(CAM_PI32)
    with np.errstate(**QUIET):
        ln = np.sqrt((r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2])
        n = r / ln[:, None]
        az = np.arctan2(n[:, 0], n[:, 2])
        alt = np.maximum(np.arcsin(np.minimum(n[:, 1], t(1))), t(0))
        u = (az + pi) / (t(2) * pi)
        v = t(0.5) + t(0.5) * np.sqrt((alt * t(2)) / pi)
    out = t(2) * lut_read(S, u, v, t)[:, :3]
    assert out.dtype == t
    return out


def sun_spot(d, material, sun_size, t=f32):
    """spot of a MISS pixel with the unit direction d [M][3]."""
    d = np.asarray(d).astype(t)
    m = np.asarray(material, f32).astype(t)
    q = m[20:23][None, :] - d
    with np.errstate(**QUIET):
        dist = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        x = np.nan_to_num(dist / t(f32(sun_size)), nan=0.0, posinf=np.inf).astype(t)
    x = clamp01(x, t)
    spot = t(1) - (x * x) * (t(3) - t(2) * x)
    return np.where(d[:, 1] <= 0, t(0), spot).astype(t)


def shade_sky(d, n, eta, foam, material, has_foam, S, t=f32):
    """ocean.h's colour of a HIT pixel with OCEAN_CAMERA_SKY_LUT: the statements of OCEAN_CAMERA_COLOR, with
    env_c = (SKY(r)_c * pi) * ke over all of r = (2 ndv) n - V."""
    d, n, eta, foam = (np.asarray(a).astype(t) for a in (d, n, eta, foam))
    m = np.asarray(material, f32).astype(t)
    pi, tiny, one, zero = t(CAM_PI32), t(TINY32), t(1), t(0)
    C, r0, fe, fd, rho, ex, ey, ke, ks = m[0:3], m[3], m[4], m[5], m[6], m[8], m[9], m[10], m[11]
    ss, ft, fc, fb, L, lc = m[12:15], m[15], m[16:19], m[19], m[20:23], m[23:26]

    def dot(a, b):
        return (a[..., 0] * b[..., 0] + a[..., 1] * b[..., 1]) + a[..., 2] * b[..., 2]

    def sat(x):
        return np.minimum(np.maximum(x, zero), one)

    V = -d
    hr = V + L[None, :]
    h = hr / np.sqrt(dot(hr, hr))[:, None]
    ndv, ndl, hdv, hdn = dot(n, V), dot(n, L[None, :]), dot(h, V), dot(h, n)
    F = r0 + ((one - r0) * np.power(one - sat(ndv), fe)) / fd
    x = one - sat(hdv)
    FH = r0 + (one - r0) * (((x * x) * (x * x)) * x)
    s = np.maximum(zero, dot(L[None, :], d))
    g = np.maximum(zero, eta) * ((s * s) * (s * s))
    r = (t(2) * ndv)[:, None] * n - V
    env = (sky_lookup(S, r, t) * pi) * ke
    refraction = C[None, :] + (g[:, None] * ss[None, :]) * lc[None, :]
    if L[1] > 0:
        den = np.maximum(one - h[:, 2] * h[:, 2], tiny)
        c2, s2 = np.maximum((h[:, 0] * h[:, 0]) / den, zero), np.maximum((h[:, 1] * h[:, 1]) / den, zero)
        nu, nv = (ex * t(10)) * (one - rho), (ey * t(10)) * (one - rho)
        D = np.sqrt((nu + one) * (nv + one)) * np.power(np.maximum(hdn, zero), nu * c2 + nv * s2)
        A = np.maximum((D * FH) / np.maximum(((t(8) * pi) * hdv) * np.maximum(ndv, ndl), tiny), zero)
        ash = lc[None, :] * A[:, None]
        a2 = (rho * rho) * (rho * rho)
        q = (sat(hdn) * sat(hdn)) * (a2 - one) + one
        N = np.maximum(a2 / np.maximum(pi * (q * q), tiny), zero)
        k = rho / t(2)
        G = np.maximum((sat(ndv) / np.maximum(sat(ndv) * (one - k) + k, tiny)) *
                       (sat(ndl) / np.maximum(sat(ndl) * (one - k) + k, tiny)), zero)
        cook = ((lc[None, :] * N[:, None]) * G[:, None]) / np.maximum((t(8) * sat(ndv)) * sat(ndl), tiny)[:, None]
    else:
        ash = cook = np.zeros((len(d), 3), t)
    reflections = env + (cook + ash * sat(ndv)[:, None]) * ks
    e = refraction + F[:, None] * (reflections - refraction)
    if has_foam:
        foamy = foam >= ft
        e = np.where(foamy[:, None], e + fb * (fc[None, :] - e), e)
    assert e.dtype == t
    return e


def sky_colours(rays, rec, hit, n, eta, foam, material, has_foam, S, sun_size, t=f32):
    """The image [M][4] of OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT from the arrays of
    tests/test_camera_abi.shading_inputs and the sky-view table S; (image, spot of every pixel)."""
    m = np.asarray(material, f32).astype(t)
    d = rays[:, 3:6]
    spot = sun_spot(d, material, sun_size, t)
    out = np.empty((len(rays), 4), t)
    out[:, :3] = sky_lookup(S, d, t) + (spot * spot)[:, None] * m[23:26][None, :]
    out[rec[:, 3] == 2, :3] = m[0:3]  # OCEAN_RAY_SUBMERGED
    out[hit, :3] = shade_sky(d[hit], n, eta, foam, material, has_foam, S, t)
    out[:, 3] = rec[:, 3]
    return out, spot
