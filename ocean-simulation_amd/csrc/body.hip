// Buoyant bodies (ocean_body_buoyancy*): M rigid bodies sharing one hull of P probes, reduced on the
// device to 32 bytes per body -- the displaced volume, its first moments about the body origin, the
// volume-weighted water normal and the worst fixed-point residual.
//
// The reference's only physics consumer is BuoyantObject.FixedUpdate -> GetWaterHeight: one probe per
// body, the volume from transform.localScale (its README: "very basic").  A host that wants hulls that
// roll and pitch puts P probes on each body; the lookups are ocean_query_surface's, and what this
// kernel adds is the transform in front of them and the reduction behind them, so that neither the
// M x P world positions nor the M x P records cross the link.  include/ocean/ocean.h states every fp32
// operation in order; per probe j of body b:
//     a = s * r_j;  t = 2 (u x a);  d = (a + qw t) + (u x t);  w = c + d            (scale, rotate, place)
//     rec = k_query_surface's record at (w.x, w.z)          (or k_query_reference's texel pick)
//     h' = h sy;  v' = ((v sx) sy) sz;  f = saturate((eta - (w.y - h'/2)) / h');  g = v' f
//     e = (d.x, (d.y - h'/2) + (f h')/2, d.z)               (centroid of the submerged part of the cell)
//     terms: g, g e, g n;  r
//
// Mapping: W = the smallest power of two >= P, capped at 64.  A wave holds 64 / W bodies of W lanes
// each, a 256-thread workgroup four such waves.  Lane l of a body walks its probes j = l, l + W, ... in
// ascending order (the trip count, ceil(P / W), is uniform over the launch) and adds its terms onto
// accumulators that start from +0; then a segmented xor butterfly of width W (__shfl_xor with s = W/2,
// ..., 1: the partner l xor s stays inside the segment because s < W) leaves every lane of the segment
// with the body's sums in the summation order the header defines, and lane 0 stores two float4.
// Lanes whose body is >= M or whose probe is >= P skip the loads, the sampling and the store, never a
// shuffle: every lane of every wave executes every __shfl_xor.
//
// No LDS, no atomics, no inline assembly.  The taps are the query kernel's: 4 texels per cascade and
// step through L1 / L2 / Infinity Cache, each step depending on the one before (latency bound, no
// roofline claimed); one body of 4 096 probes is 64 sequential chunks on one wave, by definition of
// the summation order.
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// hull float[P][5] = (rx, ry, rz, h, v); bodies float[M][10] = (c, q, s); out[2 b], out[2 b + 1] = record b.
template <int W>
__global__ __launch_bounds__(256) void k_body_buoyancy(DevView v, int tile, int mode, int iterations,
                                                       const float* __restrict__ hull, int probes,
                                                       const float* __restrict__ bodies, int count,
                                                       float4* __restrict__ out) {
    constexpr int kBodies = 256 / W;  // bodies per workgroup
    const int l = (int)(threadIdx.x % W);
    const size_t b = (size_t)blockIdx.x * kBodies + threadIdx.x / W;
    const bool live = b < (size_t)count;
    float cx = 0.0f, cy = 0.0f, cz = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f, qw = 1.0f, sx = 1.0f, sy = 1.0f, sz = 1.0f;
    if (live) {
        const float* B = bodies + 10 * b;
        cx = B[0], cy = B[1], cz = B[2];
        ux = B[3], uy = B[4], uz = B[5], qw = B[6];
        sx = B[7], sy = B[8], sz = B[9];
    }
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f, t4 = 0.0f, t5 = 0.0f, t6 = 0.0f, rmax = 0.0f;
    const int trips = (probes + W - 1) / W;  // the same for every lane of the launch
    for (int it = 0; it < trips; ++it) {
        const int j = it * W + l;
        if (live && j < probes) {
            const float* H = hull + 5 * (size_t)j;
            const float rx = H[0], ry = H[1], rz = H[2], h = H[3], vol = H[4];
            const float ax = sx * rx, ay = sy * ry, az = sz * rz;
            const float tx = 2.0f * (uy * az - uz * ay), ty = 2.0f * (uz * ax - ux * az), tz = 2.0f * (ux * ay - uy * ax);
            const float dx = (ax + qw * tx) + (uy * tz - uz * ty);
            const float dy = (ay + qw * ty) + (uz * tx - ux * tz);
            const float dz = (az + qw * tz) + (ux * ty - uy * tx);
            const float wx = cx + dx, wy = cy + dy, wz = cz + dz;
            float eta, r = 0.0f, nx = 0.0f, ny = 1.0f, nz = 0.0f;
            if (mode != OCEAN_QUERY_REFERENCE) {
                const float2 p = surface_fixed_point(v, tile, wx, wz, iterations);
                const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, wx, wz);
                eta = rec.at.x, r = rec.at.w, nx = rec.nf.x, ny = rec.nf.y, nz = rec.nf.z;
            } else {
                const int px = reference_texel(wx, v.n), py = reference_texel(wz, v.n);
                eta = (v.disp + (size_t)tile * v.C * v.n * v.n)[(size_t)py * v.n + px].y;  // cascade 0 of the tile
            }
            const float hs = h * sy, vs = ((vol * sx) * sy) * sz;
            const float bottom = wy - 0.5f * hs;
            const float f = fminf(fmaxf((eta - bottom) / hs, 0.0f), 1.0f);
            const float g = vs * f;
            const float ey = (dy - 0.5f * hs) + 0.5f * (f * hs);
            t0 = t0 + g;
            t1 = t1 + g * dx;
            t2 = t2 + g * ey;
            t3 = t3 + g * dz;
            t4 = t4 + g * nx;
            t5 = t5 + g * ny;
            t6 = t6 + g * nz;
            rmax = fmaxf(rmax, r);
        }
    }
#pragma unroll
    for (int s = W / 2; s > 0; s >>= 1) {  // every lane of the wave takes part; l xor s stays in the segment
        t0 = t0 + __shfl_xor(t0, s);
        t1 = t1 + __shfl_xor(t1, s);
        t2 = t2 + __shfl_xor(t2, s);
        t3 = t3 + __shfl_xor(t3, s);
        t4 = t4 + __shfl_xor(t4, s);
        t5 = t5 + __shfl_xor(t5, s);
        t6 = t6 + __shfl_xor(t6, s);
        rmax = fmaxf(rmax, __shfl_xor(rmax, s));
    }
    if (live && l == 0) {
        out[2 * b] = make_float4(t0, t1, t2, t3);
        out[2 * b + 1] = make_float4(t4, t5, t6, rmax);
    }
}

template <int W>
void launch_w(const DevView& v, int tile, int mode, int iterations, const float* hull, int probes,
              const float* bodies, int count, float* out, hipStream_t s) {
    constexpr int kBodies = 256 / W;
    // count * probes <= OCEAN_BODY_MAX_SAMPLES = 2^22 and W < 2 probes: at most 2^22 / 4 + 1 workgroups
    const unsigned g = (unsigned)(((size_t)count + kBodies - 1) / kBodies);
    launch(k_body_buoyancy<W>, dim3(g), dim3(256), 0, s, v, tile, mode, iterations, hull, probes, bodies, count,
           reinterpret_cast<float4*>(out));
}

}  // namespace

int body_segment_width(int probes) {
    int w = 1;
    while (w < probes && w < 64) w *= 2;
    return w;
}

hipError_t launch_body_buoyancy(const DevView& v, int tile, int mode, int iterations, const float* hull, int probes,
                                const float* bodies, int count, float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (probes < 1) return hipErrorInvalidValue;
    switch (body_segment_width(probes)) {
        case 1: launch_w<1>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        case 2: launch_w<2>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        case 4: launch_w<4>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        case 8: launch_w<8>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        case 16: launch_w<16>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        case 32: launch_w<32>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
        default: launch_w<64>(v, tile, mode, iterations, hull, probes, bodies, count, out, s); break;
    }
    return hipGetLastError();
}

}  // namespace ocean
