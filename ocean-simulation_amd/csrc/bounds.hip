// Surface bounds (ocean_surface_bounds*): the channel-wise min and max of every DISP slice of a tile, the
// numbers a renderer needs for the bounding box of its displaced mesh and the ray kernel (ray.hip) for the
// height no wave reaches.  Min and max do not depend on the order of the reduction, so the result is exact:
// numpy.min / numpy.max over the read-back slice, whatever the grid.
//
// Two passes, no float atomics.  Pass 1: a workgroup strides over its share of one slice with 16-byte loads
// (one texel per lane and load, a wave reads 1 KiB contiguous), each lane keeps the min and max of the four
// channels, the wave folds them with shuffles, the four waves meet in LDS and lane 0..7 of wave 0 write the
// workgroup's partial record.  Pass 2: one workgroup per slice folds that slice's partials the same way.
// The grid follows the slice: a workgroup per 8 loads of every lane, at most kBoundsMaxGroups per slice
// (N = 16: one workgroup, one load per lane; N = 4096: 256 workgroups of 256 loads per lane).
#include <math.h>

#include "ocean_internal.h"

namespace ocean {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;
constexpr int kLoadsPerLane = 8;  // a workgroup is worth launching for 8 KiB per wave

struct MinMax {
    float4 lo, hi;
};

__device__ __forceinline__ MinMax empty_bounds() {
    MinMax m;
    m.lo = make_float4(INFINITY, INFINITY, INFINITY, INFINITY);
    m.hi = make_float4(-INFINITY, -INFINITY, -INFINITY, -INFINITY);
    return m;
}

__device__ __forceinline__ void take(MinMax& m, float4 lo, float4 hi) {
    m.lo = make_float4(fminf(m.lo.x, lo.x), fminf(m.lo.y, lo.y), fminf(m.lo.z, lo.z), fminf(m.lo.w, lo.w));
    m.hi = make_float4(fmaxf(m.hi.x, hi.x), fmaxf(m.hi.y, hi.y), fmaxf(m.hi.z, hi.z), fmaxf(m.hi.w, hi.w));
}

__device__ __forceinline__ float4 shfl_xor4(float4 a, int s) {
    return make_float4(__shfl_xor(a.x, s, 64), __shfl_xor(a.y, s, 64), __shfl_xor(a.z, s, 64), __shfl_xor(a.w, s, 64));
}

// The workgroup's bounds in every lane of wave 0 (the other waves return their own wave's).
__device__ __forceinline__ MinMax fold_workgroup(MinMax m) {
    __shared__ float4 part[kWaves][2];
    for (int s = 32; s >= 1; s >>= 1) take(m, shfl_xor4(m.lo, s), shfl_xor4(m.hi, s));
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    if (lane == 0) {
        part[wave][0] = m.lo;
        part[wave][1] = m.hi;
    }
    __syncthreads();
    if (wave == 0)
        for (int w = 1; w < kWaves; ++w) take(m, part[w][0], part[w][1]);
    return m;
}

// Record layout (ocean.h): (min x, min y, min z, min w, max x, max y, max z, max w).
__device__ __forceinline__ void store_record(float4* rec, const MinMax& m) {
    if (threadIdx.x == 0) {
        rec[0] = m.lo;
        rec[1] = m.hi;
    }
}

// grid (groups, C): workgroup (g, c) reduces the texels g * 256 + lane + k * groups * 256 of slice
// tile * C + c into partial[c * groups + g].
__global__ __launch_bounds__(kThreads) void k_bounds_partial(const float4* __restrict__ disp, int tile, int C,
                                                             unsigned texels, float4* __restrict__ partial) {
    const int c = blockIdx.y;
    const float4* slice = disp + (size_t)(tile * C + c) * texels;
    MinMax m = empty_bounds();
    const unsigned stride = gridDim.x * kThreads;
    for (unsigned i = blockIdx.x * kThreads + threadIdx.x; i < texels; i += stride) {
        const float4 t = slice[i];
        take(m, t, t);
    }
    m = fold_workgroup(m);
    store_record(partial + 2 * ((size_t)c * gridDim.x + blockIdx.x), m);
}

// grid (C): workgroup c folds partial[c * groups .. + groups) into out[c].
__global__ __launch_bounds__(kThreads) void k_bounds_reduce(const float4* __restrict__ partial, int groups,
                                                            float4* __restrict__ out) {
    const int c = blockIdx.x;
    MinMax m = empty_bounds();
    for (int g = threadIdx.x; g < groups; g += kThreads) {
        const float4* p = partial + 2 * ((size_t)c * groups + g);
        take(m, p[0], p[1]);
    }
    m = fold_workgroup(m);
    store_record(out + 2 * (size_t)c, m);
}

}  // namespace

size_t bounds_partial_floats(int C) { return (size_t)kBoundsMaxGroups * C * 8; }

hipError_t launch_surface_bounds(const DevView& v, int tile, float* partial, float* out, hipStream_t s) {
    const unsigned texels = (unsigned)v.n * (unsigned)v.n;  // N <= 4096: 2^24 at most
    const unsigned want = (texels + kThreads * kLoadsPerLane - 1) / (kThreads * kLoadsPerLane);
    const int groups = (int)(want < 1u ? 1u : want > (unsigned)kBoundsMaxGroups ? (unsigned)kBoundsMaxGroups : want);
    launch(k_bounds_partial, dim3(groups, v.C), dim3(kThreads), 0, s, (const float4*)v.disp, tile, v.C, texels,
           reinterpret_cast<float4*>(partial));
    launch(k_bounds_reduce, dim3(v.C), dim3(kThreads), 0, s, (const float4*)partial, groups,
           reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
