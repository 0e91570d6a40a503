// Mesh hulls (ocean_body_hydrostatics*): M rigid bodies sharing one triangle mesh of V vertices and T triangles,
// reduced on the device to 64 bytes per body -- the hydrostatic pressure integrated over the wetted part of every
// triangle (force, torque about the body origin, wetted area and its first moment, the sum of the vertical area
// vectors), the draught, the worst fixed-point residual and the counts of wet triangles and vertices.
//
// The probe hulls of body.hip are vertical columns: no side, no horizontal force, no wetted area.  A mesh hull samples
// the water over its vertices, clips every triangle at the waterline and integrates the depth, which is linear over a
// clipped piece, exactly.  include/ocean/ocean.h states every fp32 operation in order.
//
// Mapping: one 256-thread workgroup per body.
//   Phase 1  thread l places vertices i = l, l + 256, ... (the scale, rotation and translation of body.hip), takes the
//            surface query's record over each (surface_fixed_point, sample_cascades, surface_record of sample_filter.h:
//            the same functions, not a copy; the taps of DERIV and TURB that the record would need feed nothing here,
//            so the compiler is free to drop them), and writes (d.x, d.y, d.z, z) as one float4 into LDS.  So a vertex is
//            sampled once, not once per incident triangle (about six times on a closed mesh): the sampling is the
//            expensive part, (K + 1) x C dependent bilinear taps through L1 / L2 / Infinity Cache.  The dynamic LDS is
//            16 V bytes (32 KiB at the cap of 2048), so a small hull keeps the workgroups per CU that its 7.5 KiB of
//            static reduction space allows.  A workgroup barrier follows.
//   Phase 2  thread l walks triangles k = l, l + 256, ... in ascending order: three indices (clamped into [0, V), so a
//            device-form caller's bad index never reads outside the vertex array), three float4 from LDS, the clip,
//            and the terms of one or two pieces added onto accumulators that start from +0.
//   Reduction  the rounds s = 128 and s = 64 of the header's xor butterfly go through LDS (the upper half stores, the
//            lower half adds: t_l + t_(l xor s) is commutative, and only lane 0's result is stored), the rounds
//            s = 32 ... 1 through __shfl_xor.  Every lane of every wave executes every barrier and every shuffle; only
//            the loads, the sampling, the LDS traffic of the two halves and the store are predicated (the discipline
//            of body.hip).  Thread 0 stores four float4.
//
// The LDS gather: ds_read_b128 serves a wave in four groups of 16 lanes over the 16 slots of 16 B of a 256-B bank row,
// and a float4 at an arbitrary vertex id lands in slot id mod 16.  Sixteen random ids into sixteen slots put about
// three on the fullest one, so a gather of a triangle soup is expected to cost about 3 x its conflict-free 4 cycles;
// a structured mesh, whose neighbouring triangles share vertices (identical addresses broadcast), less.  Three gathers
// per triangle against (K + 1) x C x 4 texel loads per vertex: the conflicts are expected to stay far below the
// sampling latency, and no swizzle is applied (a vertex id has no structure to swizzle on).  Not measured by counter.
//
// No atomics, no inline assembly.  Packing several small hulls into one workgroup is left out on purpose: a
// 12-triangle box uses 8 lanes of phase 1 and 12 of phase 2 (docs/MEASUREMENTS.md has what that costs per body).
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

struct V3 {
    float x, y, z;
};

// (a x b) as ocean.h writes it.
__device__ __forceinline__ V3 cross3(V3 a, V3 b) {
    return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
}

// X + (zx / (zx - zy)) * (Y - X): where the edge from the wet X to the dry Y meets the waterline (zx > 0 >= zy, so
// the divisor is positive).
__device__ __forceinline__ V3 waterline(V3 X, float zx, V3 Y, float zy) {
    const float t = zx / (zx - zy);
    return {X.x + t * (Y.x - X.x), X.y + t * (Y.y - X.y), X.z + t * (Y.z - X.z)};
}

// The fifteen terms of a record, in its order; two of them (the residual and the draught) are maxima, not sums.
constexpr int kTerms = 15;
__device__ __forceinline__ bool is_max(int q) { return q == 7 || q == 12; }
__device__ __forceinline__ float combine(int q, float a, float b) { return is_max(q) ? fmaxf(a, b) : a + b; }

// One wet piece (Q0, Q1, Q2; y0, y1, y2) onto the lane's accumulators.
__device__ __forceinline__ void add_piece(float* t, V3 Q0, V3 Q1, V3 Q2, float y0, float y1, float y2) {
    const V3 e1 = {Q1.x - Q0.x, Q1.y - Q0.y, Q1.z - Q0.z}, e2 = {Q2.x - Q0.x, Q2.y - Q0.y, Q2.z - Q0.z};
    const V3 cr = cross3(e1, e2);
    const V3 Av = {0.5f * cr.x, 0.5f * cr.y, 0.5f * cr.z};
    const float S = (y0 + y1) + y2;
    const float p = S / 3.0f;
    const float w0 = y0 + S, w1 = y1 + S, w2 = y2 + S;
    const V3 Mo = {((Q0.x * w0 + Q1.x * w1) + Q2.x * w2) / 12.0f, ((Q0.y * w0 + Q1.y * w1) + Q2.y * w2) / 12.0f,
                   ((Q0.z * w0 + Q1.z * w1) + Q2.z * w2) / 12.0f};
    const V3 mc = cross3(Mo, Av);
    const float ar = sqrtf((Av.x * Av.x + Av.y * Av.y) + Av.z * Av.z);
    t[0] = t[0] + -(p * Av.x);
    t[1] = t[1] + -(p * Av.y);
    t[2] = t[2] + -(p * Av.z);
    t[3] = t[3] + ar;
    t[4] = t[4] + -mc.x;
    t[5] = t[5] + -mc.y;
    t[6] = t[6] + -mc.z;
    t[8] = t[8] + ar * (((Q0.x + Q1.x) + Q2.x) / 3.0f);
    t[9] = t[9] + ar * (((Q0.y + Q1.y) + Q2.y) / 3.0f);
    t[10] = t[10] + ar * (((Q0.z + Q1.z) + Q2.z) / 3.0f);
    t[14] = t[14] + Av.y;
}

// vertices float[V][3], triangles int[T][3], bodies float[M][10] = (c, q, s); out[4 b .. 4 b + 3] = record b.
// Dynamic LDS: float4[V].  One workgroup per body (gridDim.x = count).
__global__ __launch_bounds__(256) void k_body_hydrostatics(DevView v, int tile, int iterations,
                                                           const float* __restrict__ vertices, int nverts,
                                                           const int* __restrict__ triangles, int ntris,
                                                           const float* __restrict__ bodies, float4* __restrict__ out) {
    extern __shared__ float4 placed[];       // (d, z) per vertex
    __shared__ float red[kTerms][128];       // the rounds s = 128 and s = 64
    const int l = (int)threadIdx.x;
    const size_t b = blockIdx.x;
    const float* B = bodies + 10 * b;
    const float cx = B[0], cy = B[1], cz = B[2], ux = B[3], uy = B[4], uz = B[5], qw = B[6];
    const float sx = B[7], sy = B[8], sz = B[9];

    float t[kTerms];
#pragma unroll
    for (int q = 0; q < kTerms; ++q) t[q] = 0.0f;

    for (int i = l; i < nverts; i += 256) {
        const float* R = vertices + 3 * (size_t)i;
        const float ax = sx * R[0], ay = sy * R[1], az = sz * R[2];
        const float tx = 2.0f * (uy * az - uz * ay), ty = 2.0f * (uz * ax - ux * az), tz = 2.0f * (ux * ay - uy * ax);
        const float dx = (ax + qw * tx) + (uy * tz - uz * ty);
        const float dy = (ay + qw * ty) + (uz * tx - ux * tz);
        const float dz = (az + qw * tz) + (ux * ty - uy * tx);
        const float wx = cx + dx, wy = cy + dy, wz = cz + dz;
        const float2 p = surface_fixed_point(v, tile, wx, wz, iterations);
        const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, wx, wz);
        const float z = rec.at.x - wy;
        placed[i] = make_float4(dx, dy, dz, z);
        t[7] = fmaxf(t[7], rec.at.w);
        t[12] = fmaxf(t[12], z);
        if (z > 0.0f) t[13] = t[13] + 1.0f;
    }
    __syncthreads();

    const int last = nverts - 1;
    for (int k = l; k < ntris; k += 256) {
        const int* I = triangles + 3 * (size_t)k;
        const float4 a0 = placed[min(max(I[0], 0), last)];
        const float4 a1 = placed[min(max(I[1], 0), last)];
        const float4 a2 = placed[min(max(I[2], 0), last)];
        const bool w0 = a0.w > 0.0f, w1 = a1.w > 0.0f, w2 = a2.w > 0.0f;
        const int m = (int)w0 + (int)w1 + (int)w2;
        if (m == 0) continue;
        t[11] = t[11] + 1.0f;
        // the cyclic rotation that puts the lone wet vertex (m = 1) first, or the lone dry one (m = 2) last
        const int first = m == 1 ? (w0 ? 0 : w1 ? 1 : 2) : m == 2 ? (!w2 ? 0 : !w0 ? 1 : 2) : 0;
        const float4 fa = first == 0 ? a0 : first == 1 ? a1 : a2;
        const float4 fb = first == 0 ? a1 : first == 1 ? a2 : a0;
        const float4 fc = first == 0 ? a2 : first == 1 ? a0 : a1;
        const V3 A = {fa.x, fa.y, fa.z}, Bv = {fb.x, fb.y, fb.z}, C = {fc.x, fc.y, fc.z};
        const float zA = fa.w, zB = fb.w, zC = fc.w;
        if (m == 3) {
            add_piece(t, A, Bv, C, zA, zB, zC);
        } else if (m == 1) {
            const V3 AB = waterline(A, zA, Bv, zB), AC = waterline(A, zA, C, zC);
            add_piece(t, A, AB, AC, zA, 0.0f, 0.0f);
        } else {
            const V3 BC = waterline(Bv, zB, C, zC), CA = waterline(A, zA, C, zC);
            add_piece(t, A, Bv, BC, zA, zB, 0.0f);
            add_piece(t, A, BC, CA, zA, 0.0f, 0.0f);
        }
    }

    // s = 128: lanes 128..255 hand their sums to lanes 0..127
    if (l >= 128) {
#pragma unroll
        for (int q = 0; q < kTerms; ++q) red[q][l - 128] = t[q];
    }
    __syncthreads();
    if (l < 128) {
#pragma unroll
        for (int q = 0; q < kTerms; ++q) t[q] = combine(q, t[q], red[q][l]);
    }
    __syncthreads();
    // s = 64: lanes 64..127 hand theirs to lanes 0..63
    if (l >= 64 && l < 128) {
#pragma unroll
        for (int q = 0; q < kTerms; ++q) red[q][l - 64] = t[q];
    }
    __syncthreads();
    if (l < 64) {
#pragma unroll
        for (int q = 0; q < kTerms; ++q) t[q] = combine(q, t[q], red[q][l]);
    }
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) {  // every lane of every wave takes part
#pragma unroll
        for (int q = 0; q < kTerms; ++q) t[q] = combine(q, t[q], __shfl_xor(t[q], s));
    }
    if (l == 0) {
        out[4 * b] = make_float4(t[0], t[1], t[2], t[3]);
        out[4 * b + 1] = make_float4(t[4], t[5], t[6], t[7]);
        out[4 * b + 2] = make_float4(t[8], t[9], t[10], t[11]);
        out[4 * b + 3] = make_float4(t[12], t[13], t[14], 0.0f);
    }
}

}  // namespace

hipError_t launch_body_hydrostatics(const DevView& v, int tile, int iterations, const float* vertices, int nverts,
                                    const int* triangles, int ntris, const float* bodies, int count, float* out,
                                    hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (nverts < 1 || nverts > OCEAN_HULL_MAX_VERTICES || ntris < 1 || ntris > OCEAN_HULL_MAX_TRIANGLES)
        return hipErrorInvalidValue;
    // count * nverts <= OCEAN_BODY_MAX_SAMPLES = 2^22: at most 2^22 workgroups
    launch(k_body_hydrostatics, dim3((unsigned)count), dim3(256), (uint32_t)nverts * (uint32_t)sizeof(float4), s, v, tile,
           iterations, vertices, nverts, triangles, ntris, bodies, reinterpret_cast<float4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
