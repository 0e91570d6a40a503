// World sampling of the texture-out contract (ocean_sample_world).
//
// The reference's consumer, Water.shader, reads the cascade textures at world
// positions: the Domain stage sums the displacement of every cascade sampled at
// uv = worldXZ / _Wavelengths[i] (:320-326), the Fragment stage sums derivatives and
// 1 - saturate(turbulence.x) the same way (:338-344) and builds the normal from the
// summed derivatives (:346-347).  The RenderTextures are Repeat-wrapped and
// trilinear-filtered (WaterBody.cs:112-113); the displacement array has no mips
// (:227), derivatives and turbulence do (:228-229).
//
// One lane per query point.  Filtering is stated exactly (the GPU's texture units
// round their weights in ways Unity does not specify, so this is this library's
// definition, restated in fp32 by oracle.sample_world; the code is sample_filter.h,
// shared with the surface queries of query.hip):
//   level texture of side m, uv = (x / L, z / L):  sx = u * m - 0.5, sy = v * m - 0.5;
//   i = floor(s), f = s - floor(s); texel columns i mod m, i + 1 mod m (Repeat), rows alike;
//   bilinear = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy), lerp(a, b, f) = a + f (b - a);
//   trilinear (DERIV, TURB with OCEAN_F_MIPS): lod clamped to [0, log2 N],
//   lerp(level floor(lod), level floor(lod) + 1, lod - floor(lod)); without mip chains
//   and for DISP, level 0.
// Random gathers of 4-16 texels per cascade: L2 / Infinity-Cache latency bound, not
// part of the frame (no roofline claimed).
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// Point i: (world x, world z, lod) -> out[i] = {(Dx, Dy, Dz, turbulence), (Dyx, Dyz, Dxx, Dzz), normal}.
__global__ __launch_bounds__(256) void k_sample_world(DevView v, int tile, const float* __restrict__ pts, int count,
                                                      float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float x = pts[3 * (size_t)i], z = pts[3 * (size_t)i + 1], lod = pts[3 * (size_t)i + 2];
    const WorldSample w = sample_cascades(v, tile, x, z, lod);
    const float4 disp = w.disp, deriv = w.deriv;
    const float turb = w.turb;
    out[3 * (size_t)i] = make_float4(disp.x, disp.y, disp.z, turb);
    out[3 * (size_t)i + 1] = deriv;
    out[3 * (size_t)i + 2] = normal_from_deriv(deriv.x, deriv.y, deriv.z, deriv.w);  // :346-347
}

}  // namespace

hipError_t launch_sample_world(const DevView& v, int tile, const float* pts, int count, float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const unsigned g = (unsigned)((count + 255) / 256);
    launch(k_sample_world, dim3(g), dim3(256), 0, s, v, tile, pts, count, reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
