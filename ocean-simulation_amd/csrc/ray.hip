// Ray casts against the ocean surface (ocean_raycast*): where a ray meets the water, for impacts, picking,
// line-of-sight checks and range sensors.  include/ocean/ocean.h has the definition: a fixed march over S + 1
// nodes, B bisections of the first interval that crosses, then the surface query's record at the point met.
//
// One lane per ray, no LDS.  The march itself, with its one evaluation site and its air skip, is ray_march.h,
// which the camera views (view.hip) run too.
#include "ocean_internal.h"
#include "ray_march.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// Ray i: (ox, oy, oz, dx, dy, dz, t0, t1) -> out[2 i] = (t*, gap, residual, status), out[2 i + 1] = (normal, foam).
__global__ __launch_bounds__(256) void k_raycast(DevView v, int tile, int iterations, int steps, int refine,
                                                 const float* __restrict__ bounds, const float* __restrict__ rays,
                                                 int count, float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float* r = rays + 8 * (size_t)i;
    const float ox = r[0], oy = r[1], oz = r[2], dx = r[3], dy = r[4], dz = r[5], t0 = r[6], t1 = r[7];
    const RayMeet m = ray_march(v, tile, iterations, steps, refine, bounds, ox, oy, oz, dx, dy, dz, t0, t1);
    const float t = m.t;
    const int status = m.status;

    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
    const float2 p = surface_fixed_point(v, tile, px, pz, iterations);
    const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, px, pz);
    out[2 * (size_t)i] = make_float4(t, py - rec.at.x, rec.at.w, (float)status);
    out[2 * (size_t)i + 1] = rec.nf;
}

}  // namespace

hipError_t launch_raycast(const DevView& v, int tile, int iterations, int steps, int refine, const float* bounds,
                          const float* rays, int count, float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const unsigned g = (unsigned)((count + 255) / 256);
    launch(k_raycast, dim3(g), dim3(256), 0, s, v, tile, iterations, steps, refine, bounds, rays, count,
           reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
