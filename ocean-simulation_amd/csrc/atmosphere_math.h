// What the atmosphere kernels (atmosphere.hip) and the camera's sky mode (view.hip) share: the constants of
// ocean.h's statement of the atmosphere and the fp32 bilinear read of a look-up table ("LUT reads" there).
#pragma once

#include <hip/hip_runtime.h>

#include "ocean_internal.h"

namespace ocean {

constexpr float kAtmPi = 3.14159265f;         // the compute shaders' own PI
constexpr float kAtmInvGamma = 1.0f / 2.2f;   // one fp32 division

// The row part of a read at the coordinate v: the two rows and the weight between them.
struct LutRow {
    int y0, y1;
    float f;
};

// X = clamp(u * W - 0.5, 0, W - 1) of a coordinate already in [0, 1]; a NaN becomes 0 (fmaxf returns the other operand)
__device__ __forceinline__ float lut_texel(float u, int w) { return fminf(fmaxf(u * (float)w - 0.5f, 0.0f), (float)(w - 1)); }

__device__ __forceinline__ float lut_clamp01(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }

__device__ __forceinline__ LutRow lut_row(const LutView& t, float v) {
    const float y = lut_texel(lut_clamp01(v), t.h);
    LutRow r;
    r.y0 = (int)y;
    r.y1 = min(r.y0 + 1, t.h - 1);
    r.f = y - (float)r.y0;
    return r;
}

// the four taps, x first then y, each lerp as a + f * (b - a); u is clamped here
__device__ __forceinline__ float4 lut_read(const LutView& t, float u, const LutRow& row) {
    const float x = lut_texel(lut_clamp01(u), t.w);
    const int x0 = (int)x, x1 = min(x0 + 1, t.w - 1);
    const float f = x - (float)x0;
    const float4* r0 = t.texels + (size_t)row.y0 * t.w;
    const float4* r1 = t.texels + (size_t)row.y1 * t.w;
    const float4 a0 = r0[x0], b0 = r0[x1], a1 = r1[x0], b1 = r1[x1];
    const float4 lo = make_float4(a0.x + f * (b0.x - a0.x), a0.y + f * (b0.y - a0.y), a0.z + f * (b0.z - a0.z),
                                  a0.w + f * (b0.w - a0.w));
    const float4 hi = make_float4(a1.x + f * (b1.x - a1.x), a1.y + f * (b1.y - a1.y), a1.z + f * (b1.z - a1.z),
                                  a1.w + f * (b1.w - a1.w));
    return make_float4(lo.x + row.f * (hi.x - lo.x), lo.y + row.f * (hi.y - lo.y), lo.z + row.f * (hi.z - lo.z),
                       lo.w + row.f * (hi.w - lo.w));
}

// the column coordinate of a sample at the distance sr from the planet's centre (SampleTransmittanceLUT)
__device__ __forceinline__ float lut_u(const AtmosphereParams& a, float sr) {
    return (sr - a.p[0]) / (a.p[1] - a.p[0]);
}

}  // namespace ocean
