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
//
// ocean_body_dynamics* (k_body_dynamics<W>) is the same kernel with the water's velocity joined in: at the
// point p_K the fixed point ends on, the VEL taps share each cascade's Bil with the DISP and DERIV taps (4 more
// texels per cascade, no second address computation); with the body's motion (v, omega) per probe
//     vb = v + omega x e;  u = Vs(p_K) - vb;  m = |u|;  F = g u  or  g m u;  T = e x F;  wet = f > 0
// and the sums of F, T and wet and the largest m over the wet probes ride the same lanes, trip count and
// butterfly as the seven buoyancy terms; lane 0 stores four float4 (64 B per body, the first 32 B being the
// buoyancy record bit for bit).
//
// ocean_body_step* (k_body_step<W>) puts the integrator of ocean.h behind those sums and a loop of S substeps
// around both: after the butterfly every lane of a body's segment holds all fourteen sums and advances the body's
// state in its own registers, and lane 0 stores eight float4 (128 B per body: the state, then the last substep's
// record).
//
// The probe loop and the butterfly are one device function, body_wrench<W, DRAG>, that all three kernels call:
// k_body_buoyancy<W> with DRAG = false, which compiles the VEL taps, the drag terms, their accumulators and their
// shuffles out, the other two with DRAG = true.  The three launchers share one map from P to a compile-time W
// (with_segment_width, over with_constant of ocean_internal.h) and one grid size (body_groups).
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// A body's pose, float[10] = (c, q, s) at B; a lane without a body keeps the identity and loads nothing.
struct Pose {
    float cx, cy, cz, ux, uy, uz, qw, sx, sy, sz;
};

__device__ __forceinline__ Pose load_pose(const float* B, bool live) {
    Pose q = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 1.0f, 1.0f, 1.0f, 1.0f};
    if (live) {
        q.cx = B[0], q.cy = B[1], q.cz = B[2];
        q.ux = B[3], q.uy = B[4], q.uz = B[5], q.qw = B[6];
        q.sx = B[7], q.sy = B[8], q.sz = B[9];
    }
    return q;
}

// A body's motion, float[6] = (v, omega) at Mo; a lane without a body is at rest and loads nothing.
struct Motion {
    float vx, vy, vz, ox, oy, oz;
};

__device__ __forceinline__ Motion load_motion(const float* Mo, bool live) {
    Motion mo = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    if (live) {
        mo.vx = Mo[0], mo.vy = Mo[1], mo.vz = Mo[2];
        mo.ox = Mo[3], mo.oy = Mo[4], mo.oz = Mo[5];
    }
    return mo;
}

// a rotated by the quaternion (u, w): t = 2 (u x a), (a + w t) + (u x t).
struct Vec3 {
    float x, y, z;
};

__device__ __forceinline__ Vec3 rotate(float ux, float uy, float uz, float w, float ax, float ay, float az) {
    const float tx = 2.0f * (uy * az - uz * ay), ty = 2.0f * (uz * ax - ux * az), tz = 2.0f * (ux * ay - uy * ax);
    Vec3 r;
    r.x = (ax + w * tx) + (uy * tz - uz * ty);
    r.y = (ay + w * ty) + (uz * tx - ux * tz);
    r.z = (az + w * tz) + (ux * ty - uy * tx);
    return r;
}

// Probe j of a body: d (scaled, rotated), w = c + d, and the scaled cell h', v'.
struct Placed {
    float dx, dy, dz, wx, wy, wz, hs, vs;
};

__device__ __forceinline__ Placed place_probe(const Pose& q, const float* __restrict__ H) {
    const float rx = H[0], ry = H[1], rz = H[2], h = H[3], vol = H[4];
    const Vec3 d = rotate(q.ux, q.uy, q.uz, q.qw, q.sx * rx, q.sy * ry, q.sz * rz);
    Placed p;
    p.dx = d.x, p.dy = d.y, p.dz = d.z;
    p.wx = q.cx + p.dx, p.wy = q.cy + p.dy, p.wz = q.cz + p.dz;
    p.hs = h * q.sy, p.vs = ((vol * q.sx) * q.sy) * q.sz;
    return p;
}

// The submerged part of the probe's cell under the height eta: f, g = v' f and e.y of its centroid.
struct Wet {
    float f, g, ey;
};

__device__ __forceinline__ Wet submerge(const Placed& p, float eta) {
    const float bottom = p.wy - 0.5f * p.hs;
    Wet w;
    w.f = fminf(fmaxf((eta - bottom) / p.hs, 0.0f), 1.0f);
    w.g = p.vs * w.f;
    w.ey = (p.dy - 0.5f * p.hs) + 0.5f * (w.f * p.hs);
    return w;
}

// The fourteen sums and two maxima of ocean_body_dynamics, in the record's order: t0..t6 and rmax are the buoyancy
// record, then sum F, sum T, the largest relative speed on the wet hull and the number of wet probes.
struct Wrench {
    float t0, t1, t2, t3, t4, t5, t6, rmax, f0, f1, f2, q0, q1, q2, mmax, wet;
};

// A dynamics record: the Wrench as four float4 at o.
__device__ __forceinline__ void store_wrench(float4* o, const Wrench& r) {
    o[0] = make_float4(r.t0, r.t1, r.t2, r.t3);
    o[1] = make_float4(r.t4, r.t5, r.t6, r.rmax);
    o[2] = make_float4(r.f0, r.f1, r.f2, r.q0);
    o[3] = make_float4(r.q1, r.q2, r.mmax, r.wet);
}

// The probe loop and the butterfly of all three kernels for the body whose segment lane l belongs to, at the pose
// and motion given.  Every lane of every wave calls it (the __shfl_xor are executed by all), and every lane of a
// segment returns the body's sums.  DRAG = false (ocean_body_buoyancy*) reads neither vel, law nor the motion and
// leaves the second half of the Wrench at +0: no VEL tap, no drag term, no accumulator and no shuffle for them.
template <int W, bool DRAG>
__device__ __forceinline__ Wrench body_wrench(const DevView& v, const float4* __restrict__ vel, int tile, int mode,
                                              int iterations, int law, const float* __restrict__ hull, int probes,
                                              const Pose& pose, const Motion& mo, int l, bool live) {
    [[maybe_unused]] const float vx = mo.vx, vy = mo.vy, vz = mo.vz, ox = mo.ox, oy = mo.oy, oz = mo.oz;
    float t0 = 0.0f, t1 = 0.0f, t2 = 0.0f, t3 = 0.0f, t4 = 0.0f, t5 = 0.0f, t6 = 0.0f, rmax = 0.0f;
    [[maybe_unused]] float f0 = 0.0f, f1 = 0.0f, f2 = 0.0f, q0 = 0.0f, q1 = 0.0f, q2 = 0.0f, wet = 0.0f, mmax = 0.0f;
    const int trips = (probes + W - 1) / W;  // the same for every lane of the launch
    for (int it = 0; it < trips; ++it) {
        const int j = it * W + l;
        if (live && j < probes) {
            const Placed pr = place_probe(pose, hull + 5 * (size_t)j);
            float eta, r = 0.0f, nx = 0.0f, ny = 1.0f, nz = 0.0f;
            [[maybe_unused]] float4 vs;
            if (mode != OCEAN_QUERY_REFERENCE) {  // the surface branch first (docs/MEASUREMENTS.md section 15)
                const float2 p = surface_fixed_point(v, tile, pr.wx, pr.wz, iterations);
                WorldSample s;
                if constexpr (DRAG)
                    sample_cascades_vel(v, vel, tile, p.x, p.y, s, vs);
                else
                    s = sample_cascades(v, tile, p.x, p.y, 0.0f);
                const SurfaceRecord rec = surface_record(s, p, pr.wx, pr.wz);
                eta = rec.at.x, r = rec.at.w, nx = rec.nf.x, ny = rec.nf.y, nz = rec.nf.z;
            } else {
                const int px = reference_texel(pr.wx, v.n), py = reference_texel(pr.wz, v.n);
                const size_t at = (size_t)tile * v.C * v.n * v.n + (size_t)py * v.n + px;  // cascade 0 of the tile
                eta = v.disp[at].y;
                if constexpr (DRAG) vs = vel[at];
            }
            const Wet w = submerge(pr, eta);
            [[maybe_unused]] float m, Fx, Fy, Fz;  // the drag terms are formed before the sums, as the statement order
            if constexpr (DRAG) {                  // decides the dynamics kernels' machine code (MEASUREMENTS section 27)
                const float ex = pr.dx, ey = w.ey, ez = pr.dz;
                const float bx = vx + (oy * ez - oz * ey), by = vy + (oz * ex - ox * ez), bz = vz + (ox * ey - oy * ex);
                const float ux = vs.x - bx, uy = vs.y - by, uz = vs.z - bz;
                m = sqrtf((ux * ux + uy * uy) + uz * uz);
                const float sc = law == OCEAN_DRAG_QUADRATIC ? w.g * m : w.g;
                Fx = sc * ux, Fy = sc * uy, Fz = sc * uz;
            }
            t0 = t0 + w.g;
            t1 = t1 + w.g * pr.dx;
            t2 = t2 + w.g * w.ey;
            t3 = t3 + w.g * pr.dz;
            t4 = t4 + w.g * nx;
            t5 = t5 + w.g * ny;
            t6 = t6 + w.g * nz;
            rmax = fmaxf(rmax, r);
            if constexpr (DRAG) {
                const float ex = pr.dx, ey = w.ey, ez = pr.dz;
                f0 = f0 + Fx;
                f1 = f1 + Fy;
                f2 = f2 + Fz;
                q0 = q0 + (ey * Fz - ez * Fy);
                q1 = q1 + (ez * Fx - ex * Fz);
                q2 = q2 + (ex * Fy - ey * Fx);
                if (w.f > 0.0f) {
                    wet = wet + 1.0f;
                    mmax = fmaxf(mmax, m);
                }
            }
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
        if constexpr (DRAG) {
            f0 = f0 + __shfl_xor(f0, s);
            f1 = f1 + __shfl_xor(f1, s);
            f2 = f2 + __shfl_xor(f2, s);
            q0 = q0 + __shfl_xor(q0, s);
            q1 = q1 + __shfl_xor(q1, s);
            q2 = q2 + __shfl_xor(q2, s);
            mmax = fmaxf(mmax, __shfl_xor(mmax, s));
            wet = wet + __shfl_xor(wet, s);
        }
    }
    return {t0, t1, t2, t3, t4, t5, t6, rmax, f0, f1, f2, q0, q1, q2, mmax, wet};
}

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
    const Pose pose = load_pose(bodies + 10 * b, live);
    const Wrench r = body_wrench<W, false>(v, nullptr, tile, mode, iterations, 0, hull, probes, pose, Motion{}, l, live);
    if (live && l == 0) {
        out[2 * b] = make_float4(r.t0, r.t1, r.t2, r.t3);
        out[2 * b + 1] = make_float4(r.t4, r.t5, r.t6, r.rmax);
    }
}

// ocean_body_dynamics*: the buoyancy record and, beside it, the drag of the water's velocity relative to the
// hull, summed over the wet probes.  motion float[M][6] = (v, omega); out[4 b .. 4 b + 3] = record b (64 B).
// The same mapping, trip count and butterfly as k_body_buoyancy<W>: fourteen sums and two maxima per lane.
template <int W>
__global__ __launch_bounds__(256) void k_body_dynamics(DevView v, const float4* __restrict__ vel, int tile, int mode,
                                                       int iterations, int law, const float* __restrict__ hull,
                                                       int probes, const float* __restrict__ bodies,
                                                       const float* __restrict__ motion, int count,
                                                       float4* __restrict__ out) {
    constexpr int kBodies = 256 / W;  // bodies per workgroup
    const int l = (int)(threadIdx.x % W);
    const size_t b = (size_t)blockIdx.x * kBodies + threadIdx.x / W;
    const bool live = b < (size_t)count;
    const Pose pose = load_pose(bodies + 10 * b, live);
    const Motion mo = load_motion(motion + 6 * b, live);
    const Wrench r = body_wrench<W, true>(v, vel, tile, mode, iterations, law, hull, probes, pose, mo, l, live);
    if (live && l == 0) store_wrench(out + 4 * b, r);
}

// ocean_body_step*: `substeps` substeps of the integrator ocean.h states, each behind the wrench of
// ocean_body_dynamics at the state it starts from, over one frame of water.  state float[M][32] = (c, q, s, v, omega,
// 16 ignored); props float[M][4] = (im, jx, jy, jz); sp = (h, g, B, kd, kt, la, aa, 0), uniform; out[8 b .. 8 b + 7] =
// the state after the last substep (four float4) and that substep's dynamics record (four float4).
// The mapping of k_body_dynamics<W>.  State and props stay in registers over the substeps; substeps is uniform, so
// every lane of every wave executes every __shfl_xor of every substep.  After the butterfly every lane of a segment
// holds the body's sums and integrates redundantly: no broadcast, no branch on the lane.  `out` may be `state`
// (neither is __restrict__): only body b's lanes touch record b, all of them load it here before lane 0 stores it.
template <int W>
__global__ __launch_bounds__(256) void k_body_step(DevView v, const float4* __restrict__ vel, int tile, int mode,
                                                   int iterations, int law, int substeps, BodyStepParams sp,
                                                   const float* __restrict__ hull, int probes,
                                                   const float* __restrict__ props, const float* state, int count,
                                                   float4* out) {
    constexpr int kBodies = 256 / W;  // bodies per workgroup
    const int l = (int)(threadIdx.x % W);
    const size_t b = (size_t)blockIdx.x * kBodies + threadIdx.x / W;
    const bool live = b < (size_t)count;
    Pose pose = load_pose(state + 32 * b, live);
    Motion mo = load_motion(state + 32 * b + 10, live);
    float im = 0.0f, jx = 0.0f, jy = 0.0f, jz = 0.0f;
    if (live) {
        const float* Pr = props + 4 * b;
        im = Pr[0], jx = Pr[1], jy = Pr[2], jz = Pr[3];
    }
    const float h = sp.p[0], g = sp.p[1], B = sp.p[2], kd = sp.p[3], kt = sp.p[4], la = sp.p[5], aa = sp.p[6];
    const float hh = 0.5f * h;
    Wrench r = {};
    for (int step = 0; step < substeps; ++step) {
        r = body_wrench<W, true>(v, vel, tile, mode, iterations, law, hull, probes, pose, mo, l, live);
        const float ax = im * (kd * r.f0), ay = im * (B * r.t0 + kd * r.f1) - g, az = im * (kd * r.f2);
        const float tx = kt * r.q0 - B * r.t3, ty = kt * r.q1, tz = kt * r.q2 + B * r.t1;
        const Vec3 tb = rotate(-pose.ux, -pose.uy, -pose.uz, pose.qw, tx, ty, tz);  // the torque in the body frame
        const Vec3 al = rotate(pose.ux, pose.uy, pose.uz, pose.qw, jx * tb.x, jy * tb.y, jz * tb.z);
        float vx = mo.vx + h * ax, vy = mo.vy + h * ay, vz = mo.vz + h * az;
        float ox = mo.ox + h * al.x, oy = mo.oy + h * al.y, oz = mo.oz + h * al.z;
        if (r.wet > 0.0f) {  // damping against still water while any probe is wet, from the substep's first v, omega
            vx = vx - (mo.vx * la) * h, vy = vy - (mo.vy * la) * h, vz = vz - (mo.vz * la) * h;
            ox = ox - (mo.ox * aa) * h, oy = oy - (mo.oy * aa) * h, oz = oz - (mo.oz * aa) * h;
        }
        mo = {vx, vy, vz, ox, oy, oz};
        pose.cx = pose.cx + h * vx, pose.cy = pose.cy + h * vy, pose.cz = pose.cz + h * vz;
        const float ux = pose.ux, uy = pose.uy, uz = pose.uz, qw = pose.qw;
        const float nx = ux + hh * (qw * ox + (oy * uz - oz * uy));
        const float ny = uy + hh * (qw * oy + (oz * ux - ox * uz));
        const float nz = uz + hh * (qw * oz + (ox * uy - oy * ux));
        const float nw = qw - hh * ((ox * ux + oy * uy) + oz * uz);
        const float len = sqrtf(((nx * nx + ny * ny) + nz * nz) + nw * nw);
        pose.ux = nx / len, pose.uy = ny / len, pose.uz = nz / len, pose.qw = nw / len;
    }
    if (live && l == 0) {
        out[8 * b] = make_float4(pose.cx, pose.cy, pose.cz, pose.ux);
        out[8 * b + 1] = make_float4(pose.uy, pose.uz, pose.qw, pose.sx);
        out[8 * b + 2] = make_float4(pose.sy, pose.sz, mo.vx, mo.vy);
        out[8 * b + 3] = make_float4(mo.vz, mo.ox, mo.oy, mo.oz);
        store_wrench(out + 8 * b + 4, r);
    }
}

// f(std::integral_constant<int, W>) for W = body_segment_width(probes): the one place that names the seven widths.
template <class F>
void with_segment_width(int probes, F&& f) {
    (void)with_constant<1, 2, 4, 8, 16, 32, 64>(body_segment_width(probes), f);  // it returns one of the seven
}

// Workgroups of 256 / w bodies each for `count` bodies.
// count * probes <= OCEAN_BODY_MAX_SAMPLES = 2^22 and W < 2 probes: at most 2^22 / 4 + 1 workgroups
dim3 body_groups(int count, int w) {
    const size_t per = 256 / w;
    return dim3((unsigned)(((size_t)count + per - 1) / per));
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
    with_segment_width(probes, [&](auto w) {
        launch(k_body_buoyancy<w()>, body_groups(count, w()), dim3(256), 0, s, v, tile, mode, iterations, hull, probes,
               bodies, count, reinterpret_cast<float4*>(out));
    });
    return hipGetLastError();
}

hipError_t launch_body_dynamics(const DevView& v, const float4* vel, int tile, int mode, int iterations, int law,
                                const float* hull, int probes, const float* bodies, const float* motion, int count,
                                float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (probes < 1 || !vel) return hipErrorInvalidValue;
    with_segment_width(probes, [&](auto w) {
        launch(k_body_dynamics<w()>, body_groups(count, w()), dim3(256), 0, s, v, vel, tile, mode, iterations, law, hull,
               probes, bodies, motion, count, reinterpret_cast<float4*>(out));
    });
    return hipGetLastError();
}

hipError_t launch_body_step(const DevView& v, const float4* vel, int tile, int mode, int iterations, int law, int substeps,
                            const BodyStepParams& sp, const float* hull, int probes, const float* props,
                            const float* state, int count, float* out, hipStream_t s) {
    if (count <= 0) return hipSuccess;
    if (probes < 1 || substeps < 1 || !vel) return hipErrorInvalidValue;
    with_segment_width(probes, [&](auto w) {
        launch(k_body_step<w()>, body_groups(count, w()), dim3(256), 0, s, v, vel, tile, mode, iterations, law, substeps,
               sp, hull, probes, props, state, count, reinterpret_cast<float4*>(out));
    });
    return hipGetLastError();
}

}  // namespace ocean
