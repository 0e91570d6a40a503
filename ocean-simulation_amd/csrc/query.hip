// Surface queries (ocean_query_surface*): what a buoyant body needs of the ocean at its own
// position, computed on the device so that a host moves 32 bytes per body instead of a slice.
//
// The reference answers this on the CPU: it reads displacement slice 0 back every frame
// (WaterBody.cs:288-296) and GetWaterHeight picks one texel of it (:195-209).  Two lookups:
//
//   OCEAN_QUERY_REFERENCE  GetWaterHeight's own texel pick, in fp32: world x, z mapped over
//       [-N/2, N/2] (its quirk: the texture size, not the cascade length), saturated, scaled by N,
//       truncated and clamped; the .y of that texel of cascade 0 of the tile.
//   OCEAN_QUERY_SURFACE    the height of the surface above a world (x, z).  The displacement is
//       Lagrangian: the grid point p lands at p + D_xz(p), so the water over q is Dy(p*) with
//       p* + D_xz(p*) = q.  K steps of the fixed point p <- q - D_xz(p) from p = q, on the
//       cascade-summed, bilinearly filtered displacement of ocean_sample_world (sample_filter.h),
//       then one full sample at the last p: height, normal and foam there, and the residual
//       r = |p + D_xz(p) - q|_inf that the next step would have started from.
//
// One lane per point, like k_sample_world: 4 texels per cascade and step, each step's taps
// depending on the one before, so a query is a chain of K + 1 L2 / Infinity-Cache round trips --
// latency bound at any count a host has bodies for (no roofline claimed).
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// Point i: (world x, world z) -> out[2 i] = (height, p.x, p.z, residual), out[2 i + 1] = (normal, foam).
__global__ __launch_bounds__(256) void k_query_surface(DevView v, int tile, int iterations,
                                                       const float* __restrict__ pts, int count,
                                                       float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float qx = pts[2 * (size_t)i], qz = pts[2 * (size_t)i + 1];
    const float2 p = surface_fixed_point(v, tile, qx, qz, iterations);
    const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, qx, qz);
    out[2 * (size_t)i] = rec.at;
    out[2 * (size_t)i + 1] = rec.nf;
}

// Point i: (world x, world z) -> out[2 i] = (DISP[tile * C][py][px].y, px, py, 0), out[2 i + 1] = 0.
__global__ __launch_bounds__(256) void k_query_reference(DevView v, int tile, const float* __restrict__ pts,
                                                         int count, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const int px = reference_texel(pts[2 * (size_t)i], v.n), py = reference_texel(pts[2 * (size_t)i + 1], v.n);
    const float4* slice = v.disp + (size_t)tile * v.C * v.n * v.n;  // cascade 0 of the tile
    out[2 * (size_t)i] = make_float4(slice[(size_t)py * v.n + px].y, (float)px, (float)py, 0.0f);
    out[2 * (size_t)i + 1] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
}

}  // namespace

hipError_t launch_query_surface(const DevView& v, int tile, int mode, int iterations, const float* pts, int count,
                                float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const unsigned g = (unsigned)((count + 255) / 256);
    if (mode == OCEAN_QUERY_REFERENCE)
        launch(k_query_reference, dim3(g), dim3(256), 0, s, v, tile, pts, count, reinterpret_cast<float4*>(out));
    else
        launch(k_query_surface, dim3(g), dim3(256), 0, s, v, tile, iterations, pts, count,
               reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
