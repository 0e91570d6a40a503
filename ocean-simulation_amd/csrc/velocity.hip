// Surface velocity (OCEAN_F_VELOCITY, ocean_query_velocity*): how the water moves, where the other kernels
// say where it is.  The velocity is the same inverse transform applied to dh/dt, so nothing is differenced
// in time: k_evolve_velocity forms dh/dt = i omega (A - B) from the resident H0 and WAVES with the frame's
// own phase factor and packs it as the reference packs h into DxDz and DyDxz (spectrum_math.h planes_of),
// the two planes go through the operator IFFT (fft2.hip, launched by abi_frame.cpp), and k_pack_velocity
// interleaves them into the VEL texture.  With the reference's packing VEL.xyz is the exact time derivative
// of DISP.xyz as this library computes it (include/ocean/ocean.h states every operation).
//
// Both kernels are elementwise and memory bound: 48 and 32 algorithmic bytes per texel-cascade.
// k_query_velocity is the surface query's fixed point (sample_filter.h) followed by the cascade-summed
// bilinear taps of VEL at the point it ends on: one lane per point, latency bound like k_query_surface.
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

unsigned grid_for(size_t total) {
    size_t g = (total + 255) / 256;
    return (unsigned)(g < 16384 ? (g == 0 ? 1 : g) : 16384);
}

// Texel i of every unit: H0, WAVES (16-byte loads) -> the two packed planes of dh/dt (8-byte stores).
__global__ __launch_bounds__(256) void k_evolve_velocity(const float4* __restrict__ h0,
                                                         const float4* __restrict__ waves, float2* __restrict__ v0,
                                                         float2* __restrict__ v1, size_t total, float time) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float4 h = h0[i], w = waves[i];
        const Phase e = evolve_phase(w.w, time);
        const float ex = e.ex, ey = e.ey;
        const float ax = h.x * ex - h.y * ey, ay = h.x * ey + h.y * ex;            // the two products of evolve_h
        const float bx = h.z * ex - h.w * (-ey), by = h.z * (-ey) + h.w * ex;
        const float gx = ax - bx, gy = ay - by;
        const float2 ht = make_float2(-(gy * w.w), gx * w.w);                      // dh/dt = i omega (A - B)
        const Planes4 o = planes_of(ht, w);
        v0[i] = o.p[0];
        v1[i] = o.p[1];
    }
}

// VEL[i] = (Re V0, Re V1, Im V0, Im V1): one texel per lane, 16-byte stores.  NT: streamed stores, for a
// VEL that nothing reads before the next frame has passed through the caches (OCEAN_VEL_NT=1).
template <bool NT>
__global__ __launch_bounds__(256) void k_pack_velocity(const float2* __restrict__ v0, const float2* __restrict__ v1,
                                                       float4* __restrict__ vel, size_t total) {
    for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
        const float2 a = v0[i], b = v1[i];
        if (NT) {
            const f32x4 o = {a.x, b.x, a.y, b.y};
            __builtin_nontemporal_store(o, reinterpret_cast<f32x4*>(vel + i));
        } else {
            vel[i] = make_float4(a.x, b.x, a.y, b.y);
        }
    }
}

// Point i: (world x, world z) -> out[2 i] = (Vs.xyz, residual), out[2 i + 1] = (height, p.x, p.z, Vs.w).
__global__ __launch_bounds__(256) void k_query_velocity(DevView v, const float4* __restrict__ vel, int tile,
                                                        int iterations, const float* __restrict__ pts, int count,
                                                        float4* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= count) return;
    const float qx = pts[2 * (size_t)i], qz = pts[2 * (size_t)i + 1];
    const float2 p = surface_fixed_point(v, tile, qx, qz, iterations);
    const float4 vs = sample_velocity(v, vel, tile, p.x, p.y);
    const float4 d = sample_disp(v, tile, p.x, p.y);
    out[2 * (size_t)i] = make_float4(vs.x, vs.y, vs.z, surface_residual(d, p, qx, qz));
    out[2 * (size_t)i + 1] = make_float4(d.y, p.x, p.y, vs.w);
}

}  // namespace

hipError_t launch_evolve_velocity(const DevView& v, float2* scratch, float t, hipStream_t s) {
    const size_t total = (size_t)v.n * v.n * v.units;
    launch(k_evolve_velocity, dim3(grid_for(total)), dim3(256), 0, s, (const float4*)v.h0, (const float4*)v.waves,
           scratch, scratch + total, total, t);
    return hipGetLastError();
}

hipError_t launch_pack_velocity(const DevView& v, const float2* scratch, float4* vel, bool streamed, hipStream_t s) {
    const size_t total = (size_t)v.n * v.n * v.units;
    if (streamed)
        launch(k_pack_velocity<true>, dim3(grid_for(total)), dim3(256), 0, s, scratch, scratch + total, vel, total);
    else
        launch(k_pack_velocity<false>, dim3(grid_for(total)), dim3(256), 0, s, scratch, scratch + total, vel, total);
    return hipGetLastError();
}

hipError_t launch_query_velocity(const DevView& v, const float4* vel, int tile, int iterations, const float* pts,
                                 int count, float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    const unsigned g = (unsigned)((count + 255) / 256);
    launch(k_query_velocity, dim3(g), dim3(256), 0, s, v, vel, tile, iterations, pts, count,
           reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
