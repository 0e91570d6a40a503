// The atmosphere (ocean_atmosphere, ocean_sky_update): the three look-up tables of the reference's
// AtmosphereController.cs, restated from its three compute shaders.  include/ocean/ocean.h has the definition,
// operation by operation; every statement here is one of its lines, in fp32 with one rounding per operation
// (the library is built with -ffp-contract=off), the reference's quirks kept.
//
//   k_transmittance   TransmittanceLUT.compute:25-51.  One lane per texel, 500 dependent steps of two expf: compute
//                     bound, 64 x 256 texels = 256 waves.  Runs once per ocean_atmosphere.
//   k_multiscatter    MultiscatteringLUT.compute:56-127.  One WAVE per texel: lane i marches direction i of the
//                     reference's 64 for 32 steps and adds its own ground term, and the 64 partial sums are folded by
//                     a fixed xor butterfly (the one of body.hip), so a 64 x 64 table is 4096 waves and not 64.  The
//                     result depends on neither the grid nor the scheduling: no atomics, no LDS.
//   k_skyview         SkyViewLUT.compute:83-148.  One lane per texel, a wave on an 8 x 8 texel tile (as view.hip): the
//                     per-frame kernel, 32 steps with one read of each of the other two tables.  The sun's height is
//                     the same for every texel and step, so the row taps and the row weight of both reads are formed
//                     once per lane before the loop, from kernel arguments alone (wave-uniform: scalar registers).
//
// The tables are float4 per texel (the reference's ARGBFloat), 832 KiB at the default sizes: they stay in L2, and a
// read is four 16-B taps combined in fp32 (lut_read).  A tap's indices are clamped after a NaN-proof clamp of the
// coordinate, so no input reaches outside a table.
#include "atmosphere_math.h"
#include "ocean_internal.h"

namespace ocean {
namespace {

constexpr int kTransmittanceSteps = 500;
constexpr int kSteps = 32;

struct Densities {
    float r, m, o;
};
// the three density profiles at the height h above the ground (TransmittanceLUT.compute:44-46)
__device__ __forceinline__ Densities densities(const AtmosphereParams& a, float h) {
    Densities d;
    d.r = expf((-h) / a.p[8]);
    d.m = expf((-h) / a.p[15]);
    d.o = fmaxf(0.0f, 1.0f - (h - 25000.0f) / 15000.0f);
    return d;
}
// channel c of (Rayleigh_c * d.r + Mie_c * d.m) + Ozone_c * d.o
__device__ __forceinline__ float mix3(float r, float m, float o, const Densities& d) { return (r * d.r + m * d.m) + o * d.o; }

// radius and cosine of texel (x, y) of a W x H table (TransmittanceLUT.compute:27-28)
__device__ __forceinline__ void texel_radius_mu(const AtmosphereParams& a, int x, int y, int w, int h, float* radius, float* mu) {
    const float u = ((float)x + 0.5f) / (float)w, v = ((float)y + 0.5f) / (float)h;
    *radius = u * (a.p[1] - a.p[0]) + a.p[0];
    *mu = -1.0f + v * 2.0f;
}

__global__ __launch_bounds__(256) void k_transmittance(AtmosphereParams a, int w, int h, float4* __restrict__ lut) {
    // a workgroup of four waves is a 16 x 16 texel tile, wave q its 8 x 8 quadrant
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (q & 1) * 8 + (l & 7);
    const int y = blockIdx.y * 16 + (q >> 1) * 8 + (l >> 3);
    if (x >= w || y >= h) return;
    float radius, mu;
    texel_radius_mu(a, x, y, w, h, &radius, &mu);
    const float ra = a.p[1], rp = a.p[0];
    const float disc = fmaxf(0.0f, (radius * radius) * (mu * mu - 1.0f) + ra * ra);
    const float step = fmaxf(0.0f, (-radius) * mu + sqrtf(disc)) / (float)kTransmittanceSteps;
    const float ex0 = a.p[2] + a.p[5], ex1 = a.p[3] + a.p[6], ex2 = a.p[4] + a.p[7];
    const float em0 = a.p[9] + a.p[12], em1 = a.p[10] + a.p[13], em2 = a.p[11] + a.p[14];
    const float eo0 = a.p[17] + a.p[20], eo1 = a.p[18] + a.p[21], eo2 = a.p[19] + a.p[22];
    const float two_r_mu = (2.0f * radius) * mu, r2 = radius * radius;
    float e0 = 0.0f, e1 = 0.0f, e2 = 0.0f;
    for (int i = 0; i < kTransmittanceSteps; ++i) {
        const float d = ((float)i + 0.5f) * step;
        const float sr = sqrtf((d * d + two_r_mu * d) + r2);
        const Densities dn = densities(a, sr - rp);
        e0 = e0 + mix3(ex0, em0, eo0, dn) * step;
        e1 = e1 + mix3(ex1, em1, eo1, dn) * step;
        e2 = e2 + mix3(ex2, em2, eo2, dn) * step;
    }
    lut[(size_t)y * w + x] = make_float4(expf(-e0), expf(-e1), expf(-e2), 0.0f);
}

// One step of the two 32-step marches (MultiscatteringLUT.compute:91-113, SkyViewLUT.compute:300-321): what both
// share of a sample at the distance `cur` along (dx, dy, dz) from (0, radius, 0).
struct MarchSample {
    float sr;      // the sample's distance from the planet's centre
    Densities dn;
};
__device__ __forceinline__ MarchSample march_sample(const AtmosphereParams& a, float radius, float cur, float dx, float dy,
                                                    float dz) {
    const float px = cur * dx, py = radius + cur * dy, pz = cur * dz;
    MarchSample s;
    s.sr = sqrtf((px * px + py * py) + pz * pz);
    s.dn = densities(a, s.sr - a.p[0]);
    return s;
}

__global__ __launch_bounds__(256) void k_multiscatter(AtmosphereParams a, LutView tr, int w, int h, float4* __restrict__ lut) {
    const int texel = blockIdx.x * 4 + (threadIdx.x >> 6);  // one wave per texel: the test is wave-uniform
    if (texel >= w * h) return;
    const int lane = threadIdx.x & 63;
    const int x = texel % w, y = texel / w;
    float radius, mu;
    texel_radius_mu(a, x, y, w, h, &radius, &mu);
    const float rp = a.p[0], ra = a.p[1];
    const float uniform_phase = 1.0f / (4.0f * kAtmPi);

    // direction `lane` of the 64 (:76-79)
    const float z = ((float)lane + 0.5f) / 64.0f;
    const float xy = sqrtf(1.0f - z * z);
    const float az = ((z * 8.0f) * kAtmPi) * 2.0f;
    const float dx = sinf(az) * xy, dy = cosf(az) * xy, dz = z;

    // where the ray ends (:30-46)
    const float off = (-radius) * dy;
    const float rc2 = radius * radius - off * off;
    const float p2 = rp * rp;
    const bool hit = rc2 < p2 && dy < 0.0f;
    const float end = hit ? off - sqrtf(p2 - rc2) : sqrtf(ra * ra - rc2) + off;
    const float step = end / (float)kSteps;

    const LutRow row = lut_row(tr, 0.5f + 0.5f * mu);
    const float ex[3] = {a.p[2] + a.p[5], a.p[3] + a.p[6], a.p[4] + a.p[7]};
    const float em[3] = {a.p[9] + a.p[12], a.p[10] + a.p[13], a.p[11] + a.p[14]};
    const float eo[3] = {a.p[17] + a.p[20], a.p[18] + a.p[21], a.p[19] + a.p[22]};
    float t[3] = {1.0f, 1.0f, 1.0f}, lum[3] = {0.0f, 0.0f, 0.0f}, tf[3] = {0.0f, 0.0f, 0.0f};
    float cur = step * 0.5f;
    for (int j = 0; j < kSteps; ++j) {
        const MarchSample s = march_sample(a, radius, cur, dx, dy, dz);
        const float4 tsun = lut_read(tr, lut_u(a, s.sr), row);
        const float ts[3] = {tsun.x, tsun.y, tsun.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float sc = mix3(a.p[2 + c], a.p[9 + c], a.p[17 + c], s.dn);
            const float ins = (ts[c] * sc) * uniform_phase;
            const float e = mix3(ex[c], em[c], eo[c], s.dn);
            const float nt = t[c] * expf((-e) * step);
            const float ti = (t[c] - nt) / e;
            lum[c] = lum[c] + ti * ins;
            tf[c] = tf[c] + ti * sc;
            t[c] = nt;
        }
        cur = cur + step;
    }
    if (hit) {  // the ground's own light (:120)
        const float4 tg = lut_read(tr, lut_u(a, radius), row);
        const float g[3] = {tg.x, tg.y, tg.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) lum[c] = lum[c] + ((t[c] * g[c]) * (a.p[23 + c] / kAtmPi)) * mu;
    }
    // the fixed butterfly of ocean.h: every lane of the wave takes part, and every lane ends with the sums
    for (int s = 32; s > 0; s >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            lum[c] = lum[c] + __shfl_xor(lum[c], s);
            tf[c] = tf[c] + __shfl_xor(tf[c], s);
        }
    }
    if (lane == 0)
        lut[texel] = make_float4(lum[0] / (64.0f - tf[0]), lum[1] / (64.0f - tf[1]), lum[2] / (64.0f - tf[2]), 1.0f);
}

__global__ __launch_bounds__(256) void k_skyview(AtmosphereParams a, LutView tr, LutView ms, float sunx, float suny,
                                                 float sunz, int w, int h, float4* __restrict__ lut) {
    const int q = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int x = blockIdx.x * 16 + (q & 1) * 8 + (l & 7);
    const int y = blockIdx.y * 16 + (q >> 1) * 8 + (l >> 3);
    if (x >= w || y >= h) return;
    const float rp = a.p[0], ra = a.p[1], g = a.p[16];

    // the texel's direction (:87-101); the observer stands on the ground
    const float lon = -kAtmPi + (((float)x + 0.5f) / ((float)w - 1.0f)) * (2.0f * kAtmPi);
    const float v = 1.0f - ((float)y + 0.5f) / ((float)h - 1.0f);
    const float radius = rp;
    const float horizon = sqrtf(radius * radius - rp * rp);
    const float beta = acosf(horizon / radius);
    const float zha = kAtmPi - beta;
    float lat = v * 2.0f - 1.0f;
    lat = lat * lat;
    lat = v < 0.5f ? (1.0f - lat) * zha : zha + lat * beta;
    const float sl = sinf(lat), cl = cosf(lat);
    const float dx = sinf(lon) * sl, dy = cl, dz = cosf(lon) * sl;

    // the two phase functions (:52-65, :105-108)
    const float cs = (dx * sunx + dy * suny) + dz * sunz;
    const float ray_phase = (3.0f / (16.0f * kAtmPi)) * (1.0f + cs * cs);
    const float num = (1.0f - g * g) * (1.0f + cs * cs);
    const float den = (2.0f + g * g) * powf(fabsf((1.0f + g * g) - ((2.0f * g) * cs)), 1.5f);
    const float mie_phase = ((3.0f / (8.0f * kAtmPi)) * num) / den;

    // where the ray starts and ends (:33-50, :110-112)
    const float off = (-radius) * cl;
    const float rc2 = radius * radius - off * off;
    const float p2 = rp * rp;
    const float top = sqrtf(ra * ra - rc2);
    const float start = fmaxf(0.0f, off - top);
    const float end = (rc2 < p2 && cl < 0.0f) ? off - sqrtf(p2 - rc2) : top + off;
    const float step = (end - start) / (float)kSteps;

    // both tables are read at the sun's height: one row pair and one row weight each, for every texel and step
    const float vrow = 0.5f + 0.5f * suny;
    const LutRow trow = lut_row(tr, vrow), mrow = lut_row(ms, vrow);
    const float ex[3] = {a.p[2] + a.p[5], a.p[3] + a.p[6], a.p[4] + a.p[7]};
    const float em[3] = {a.p[9] + a.p[12], a.p[10] + a.p[13], a.p[11] + a.p[14]};
    const float eo[3] = {a.p[17] + a.p[20], a.p[18] + a.p[21], a.p[19] + a.p[22]};
    float t[3] = {1.0f, 1.0f, 1.0f}, lum[3] = {0.0f, 0.0f, 0.0f};
    float cur = step * 0.5f + start;
    for (int i = 0; i < kSteps; ++i) {
        const MarchSample s = march_sample(a, radius, cur, dx, dy, dz);
        const float u = lut_u(a, s.sr);
        const float4 tsun = lut_read(tr, u, trow), msun = lut_read(ms, u, mrow);
        const float ts[3] = {tsun.x, tsun.y, tsun.z}, mm[3] = {msun.x, msun.y, msun.z};
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float rph = a.p[2 + c] * ray_phase, mph = a.p[9 + c] * mie_phase;
            float ins = ts[c] * (s.dn.r * rph + s.dn.m * mph);
            const float sc = mix3(a.p[2 + c], a.p[9 + c], a.p[17 + c], s.dn);
            ins = ins + mm[c] * sc;
            const float e = mix3(ex[c], em[c], eo[c], s.dn);
            const float nt = t[c] * expf((-e) * step);
            const float ti = (t[c] - nt) / e;
            lum[c] = lum[c] + ti * ins;
            t[c] = nt;
        }
        cur = cur + step;
    }
    lut[(size_t)y * w + x] = make_float4(powf(fabsf(lum[0]), kAtmInvGamma), powf(fabsf(lum[1]), kAtmInvGamma),
                                         powf(fabsf(lum[2]), kAtmInvGamma), 1.0f);
}

bool dims_ok(int w, int h) { return w >= 2 && h >= 2 && w <= OCEAN_ATMOSPHERE_MAX_DIM && h <= OCEAN_ATMOSPHERE_MAX_DIM; }

}  // namespace

hipError_t launch_transmittance(const AtmosphereParams& a, int w, int h, float4* lut, hipStream_t s) {
    if (!dims_ok(w, h)) return hipErrorInvalidValue;
    launch(k_transmittance, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, s, a, w, h, lut);
    return hipGetLastError();
}

hipError_t launch_multiscatter(const AtmosphereParams& a, const LutView& tr, int w, int h, float4* lut, hipStream_t s) {
    if (!dims_ok(w, h) || !dims_ok(tr.w, tr.h)) return hipErrorInvalidValue;
    launch(k_multiscatter, dim3((w * h + 3) / 4), dim3(256), 0, s, a, tr, w, h, lut);
    return hipGetLastError();
}

hipError_t launch_skyview(const AtmosphereParams& a, const LutView& tr, const LutView& ms, const float* sun, int w, int h,
                          float4* lut, hipStream_t s) {
    if (!dims_ok(w, h) || !dims_ok(tr.w, tr.h) || !dims_ok(ms.w, ms.h)) return hipErrorInvalidValue;
    launch(k_skyview, dim3((w + 15) / 16, (h + 15) / 16), dim3(256), 0, s, a, tr, ms, sun[0], sun[1], sun[2], w, h, lut);
    return hipGetLastError();
}

}  // namespace ocean
