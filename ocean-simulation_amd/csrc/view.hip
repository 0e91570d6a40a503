// Camera views of the ocean (ocean_camera*): an image of the sea from a camera of fourteen numbers, as a range
// image, a G-buffer of ray records or a shaded picture.  include/ocean/ocean.h has the definition: pixel (i, j)'s
// ray follows from the camera, meets the water where ocean_raycast says that ray does (ray_march.h: the same
// statements), and in colour mode the fragment stage of Water.shader (:336-373) is evaluated at the point met,
// with the header's headless substitutions (no shadow map, no opaque texture, a two-colour sky).  With
// OCEAN_CAMERA_SKY_LUT the sky is the atmosphere's sky-view table instead (sky_lut: SampleSkyLUT of Atmosphere.shader),
// and a miss adds the sun's disc: that image is a kernel of its own (k_camera_sky), so the other three keep their
// arguments and registers.
//
// One lane per pixel, no LDS.  A pixel is the ray kernel's chain of dependent L2 / Infinity-Cache round trips:
// latency bound, hidden by occupancy.  What the image adds is coherence: neighbouring pixels' rays pass over
// neighbouring water, so the lanes of a wave read the same texel lines when they cover a compact patch of the
// image.  A wave therefore takes an 8 x 8 pixel tile and a workgroup of four waves a 16 x 16 one; the row-linear
// mapping (64 consecutive pixels of a row per wave) is kept beside it for the comparison in docs/MEASUREMENTS.md
// (OCEAN_CAMERA_TILE=0).  The mapping decides which lane computes a pixel, never a bit of its result.
//
// The mode is a template argument: the range image needs no sample at the point met and the G-buffer none of
// the shading, so each kernel carries only its own registers.  Camera and material are kernel arguments
// (14 + 32 floats): every lane reads them from scalar registers, and there is no staged input.
#include "atmosphere_math.h"
#include "ocean_internal.h"
#include "ray_march.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

constexpr float kPi = 3.14159265358979323846f;
constexpr float kFltMin = 1.175494351e-38f;

__device__ __forceinline__ float saturate(float x) { return fminf(fmaxf(x, 0.0f), 1.0f); }
__device__ __forceinline__ float dot3(float ax, float ay, float az, float bx, float by, float bz) {
    return (ax * bx + ay * by) + az * bz;
}

// sky(r) of ocean.h, one channel: horizon + saturate(r.y) * (zenith - horizon)
__device__ __forceinline__ float sky(float horizon, float zenith, float ry) {
    return horizon + saturate(ry) * (zenith - horizon);
}

// sky(r) of ocean.h with OCEAN_CAMERA_SKY_LUT: twice the sky-view table at the direction r (any length)
__device__ __forceinline__ float3 sky_lut(const LutView& sk, float rx, float ry, float rz) {
    const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
    const float nx = rx / len, ny = ry / len, nz = rz / len;
    const float az = atan2f(nx, nz);
    const float alt = fmaxf(asinf(fminf(ny, 1.0f)), 0.0f);  // below the horizon: the horizon
    const float u = (az + kPi) / (2.0f * kPi);
    const float v = 0.5f + 0.5f * sqrtf((alt * 2.0f) / kPi);
    const float4 t = lut_read(sk, u, lut_row(sk, v));
    return make_float3(2.0f * t.x, 2.0f * t.y, 2.0f * t.z);
}

// What the bodies add to the colour of a water pixel (ocean.h, ocean_camera_scene): the body seen through the water
// and its fog, the body in the mirror, the shadow.
struct SceneTerms {
    bool through, mirrored, shadowed;
    float fog;
    float seen[3], mirror[3];  // paintc of the body seen through the water, and of the reflected one
    float sh[3], si;           // _ShadowsColor, _ShadowsIntensity
};

// The colour of a hit pixel (ocean.h, "Colour of a hit"): the ray direction d, the normal n, the wave height and
// the foam at the point met.  has_foam: the context has DERIV and TURB (not DISPLACEMENT_ONLY).
// SKY: the sky is sky_lut over `sk`, else the two-colour sky of the material.
// SCENE: with the terms of `sc` (ocean_camera_scene); without, every statement is ocean_camera's.
template <bool SKY, bool SCENE = false>
__device__ __forceinline__ float3 shade_hit(const CameraMaterial& mt, float dx, float dy, float dz, float nx, float ny,
                                            float nz, float height, float foam, bool has_foam, const LutView& sk,
                                            const SceneTerms& sc = SceneTerms{}) {
    const float* m = mt.m;
    const float r0 = m[3], rough = m[6];
    const float lx = m[20], ly = m[21], lz = m[22];
    const float vx = -dx, vy = -dy, vz = -dz;
    // the halfway vector
    const float hrx = vx + lx, hry = vy + ly, hrz = vz + lz;
    const float hl = sqrtf((hrx * hrx + hry * hry) + hrz * hrz);
    const float hx = hrx / hl, hy = hry / hl, hz = hrz / hl;
    const float ndv = dot3(nx, ny, nz, vx, vy, vz), ndl = dot3(nx, ny, nz, lx, ly, lz);
    const float hdv = dot3(hx, hy, hz, vx, vy, vz), hdn = dot3(hx, hy, hz, nx, ny, nz);
    const float sndv = saturate(ndv), sndl = saturate(ndl);
    // the two Fresnel terms
    const float fresnel = r0 + ((1.0f - r0) * powf(1.0f - sndv, m[4])) / m[5];
    const float x = 1.0f - saturate(hdv);
    const float fresnel_h = r0 + (1.0f - r0) * (((x * x) * (x * x)) * x);
    // subsurface scattering: dot(light, -V) = dot(light, d)
    const float sl = fmaxf(0.0f, dot3(lx, ly, lz, dx, dy, dz));
    const float coeff = fmaxf(0.0f, height) * ((sl * sl) * (sl * sl));
    // the sky at -reflect(V, n) = 2 dot(n, V) n - V: only its y is needed
    const float ry = (2.0f * ndv) * ny - vy;
    float env_sky[3] = {0.0f, 0.0f, 0.0f};
    if (SKY && !(SCENE && sc.mirrored)) {  // all of -reflect(V, n)
        const float3 e = sky_lut(sk, (2.0f * ndv) * nx - vx, ry, (2.0f * ndv) * nz - vz);
        env_sky[0] = e.x, env_sky[1] = e.y, env_sky[2] = e.z;
    }
    // the sun's two lobes: zero for a light at or below the horizon
    const bool sun_up = ly > 0.0f;
    float as = 0.0f, dist = 0.0f, geom = 0.0f, ctden = 1.0f;
    if (sun_up) {
        const float den = fmaxf(1.0f - hz * hz, kFltMin);
        const float cos2 = fmaxf((hx * hx) / den, 0.0f), sin2 = fmaxf((hy * hy) / den, 0.0f);
        const float nu = (m[8] * 10.0f) * (1.0f - rough), nv = (m[9] * 10.0f) * (1.0f - rough);
        const float d = sqrtf((nu + 1.0f) * (nv + 1.0f)) * powf(fmaxf(hdn, 0.0f), nu * cos2 + nv * sin2);
        as = fmaxf((d * fresnel_h) / fmaxf(((8.0f * kPi) * hdv) * fmaxf(ndv, ndl), kFltMin), 0.0f);
        const float alpha = rough * rough, a2 = alpha * alpha;
        const float ndh = saturate(hdn);
        const float q = (ndh * ndh) * (a2 - 1.0f) + 1.0f;
        dist = fmaxf(a2 / fmaxf(kPi * (q * q), kFltMin), 0.0f);
        const float k = rough / 2.0f;
        const float gv = sndv / fmaxf(sndv * (1.0f - k) + k, kFltMin), gl = sndl / fmaxf(sndl * (1.0f - k) + k, kFltMin);
        geom = fmaxf(gv * gl, 0.0f);
        ctden = fmaxf((8.0f * sndv) * sndl, kFltMin);
    }
    const bool foamy = has_foam && foam >= m[15];
    float out[3];
    for (int c = 0; c < 3; ++c) {
        const float light = m[23 + c];
        float base = m[c];
        if (SCENE && sc.through) base = m[c] + sc.fog * (sc.seen[c] - m[c]);
        const float refr = base + (coeff * m[12 + c]) * light;
        float src = SKY ? env_sky[c] : sky(m[26 + c], m[29 + c], ry);
        if (SCENE && sc.mirrored) src = sc.mirror[c];
        const float env = (src * kPi) * m[10];
        const float cook = sun_up ? ((light * dist) * geom) / ctden : 0.0f;
        const float ashk = sun_up ? light * as : 0.0f;
        const float refl = SCENE && sc.shadowed ? env : env + (cook + ashk * sndv) * m[11];
        float e = refr + fresnel * (refl - refr);
        if (SCENE && sc.shadowed) e = e + sc.si * (sc.sh[c] - e);
        if (foamy) e = e + m[19] * (m[16 + c] - e);
        out[c] = e;
    }
    return make_float3(out[0], out[1], out[2]);
}

// d of ocean.h for the pixel at (fi, fj): the camera's direction through it, normalised.
struct Vec3 {
    float x, y, z;
};
__device__ __forceinline__ Vec3 pixel_direction(const CameraRays& cam, float fi, float fj) {
    const float rx = (cam.c[3] + fi * cam.c[6]) + fj * cam.c[9];
    const float ry = (cam.c[4] + fi * cam.c[7]) + fj * cam.c[10];
    const float rz = (cam.c[5] + fi * cam.c[8]) + fj * cam.c[11];
    const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
    Vec3 d;
    d.x = rx / len, d.y = ry / len, d.z = rz / len;
    return d;
}

// Element k of `out` for a pixel whose ray (o, d) met the water as `m` says (HIT, MISS or SUBMERGED): ocean_camera's
// pixel in MODE.  SKY (colour mode only): the sky and the sun's disc of OCEAN_CAMERA_SKY_LUT over `sk`.
template <int MODE, bool SKY>
__device__ __forceinline__ void water_pixel(const DevView& v, int tile, int iterations, const CameraMaterial& mt, float ox,
                                            float oy, float oz, float dx, float dy, float dz, const RayMeet& m, size_t k,
                                            float* __restrict__ out, const LutView& sk, float sun_size) {
    const float t = m.t;
    if (MODE == OCEAN_CAMERA_RANGE) {
        out[k] = m.status == OCEAN_RAY_MISS ? __builtin_inff() : t;
        return;
    }
    if (MODE == OCEAN_CAMERA_COLOR && m.status != OCEAN_RAY_HIT) {
        float4 c;
        if (m.status == OCEAN_RAY_MISS && SKY) {
            const float3 e = sky_lut(sk, dx, dy, dz);
            float spot = 0.0f;  // SunShape (Atmosphere.shader:57-63)
            if (dy > 0.0f) {
                const float ex = mt.m[20] - dx, ey = mt.m[21] - dy, ez = mt.m[22] - dz;
                const float dist = sqrtf((ex * ex + ey * ey) + ez * ez);
                const float x = saturate(dist / sun_size);
                spot = 1.0f - (x * x) * (3.0f - 2.0f * x);
            }
            const float s2 = spot * spot;
            c = make_float4(e.x + s2 * mt.m[23], e.y + s2 * mt.m[24], e.z + s2 * mt.m[25], 0.0f);
        } else if (m.status == OCEAN_RAY_MISS)
            c = make_float4(sky(mt.m[26], mt.m[29], dy), sky(mt.m[27], mt.m[30], dy), sky(mt.m[28], mt.m[31], dy), 0.0f);
        else
            c = make_float4(mt.m[0], mt.m[1], mt.m[2], 0.0f);
        c.w = (float)m.status;
        reinterpret_cast<float4*>(out)[k] = c;
        return;
    }
    const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
    const float2 p = surface_fixed_point(v, tile, px, pz, iterations);
    if (MODE == OCEAN_CAMERA_HITS) {
        const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, px, pz);
        float4* o = reinterpret_cast<float4*>(out) + 2 * k;
        o[0] = make_float4(t, py - rec.at.x, rec.at.w, (float)m.status);
        o[1] = rec.nf;
    } else {
        const WorldSample s = sample_cascades(v, tile, p.x, p.y, t * mt.m[7]);
        const float4 n = normal_from_deriv(s.deriv.x, s.deriv.y, s.deriv.z, s.deriv.w);  // (0, 1, 0) without DERIV
        const float3 c = shade_hit<SKY>(mt, dx, dy, dz, n.x, n.y, n.z, s.disp.y, s.turb, v.deriv != nullptr, sk);
        reinterpret_cast<float4*>(out)[k] = make_float4(c.x, c.y, c.z, (float)m.status);
    }
}

// Pixel (i, j) -> element k = j * width + i of `out`.  TILED: a workgroup is a 16 x 16 pixel tile, wave w its
// 8 x 8 quadrant (w & 1, w >> 1), lane l the pixel (l & 7, l >> 3) of it; else 256 consecutive k per workgroup.
template <int MODE, bool TILED, bool SKY>
__device__ __forceinline__ void camera_pixel(const DevView& v, int tile, int iterations, int steps, int refine,
                                             const float* __restrict__ bounds, const CameraRays& cam,
                                             const CameraMaterial& mt, int width, int height, float* __restrict__ out,
                                             const LutView& sk, float sun_size) {
    int i, j;
    if (TILED) {
        const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
        i = blockIdx.x * 16 + (w & 1) * 8 + (l & 7);
        j = blockIdx.y * 16 + (w >> 1) * 8 + (l >> 3);
    } else {
        const int lin = blockIdx.x * 256 + threadIdx.x;  // < 2^22 + 256
        i = lin % width;
        j = lin / width;
    }
    if (i >= width || j >= height) return;
    const size_t k = (size_t)j * width + i;
    const Vec3 d = pixel_direction(cam, (float)i, (float)j);
    const float ox = cam.c[0], oy = cam.c[1], oz = cam.c[2];
    const RayMeet m = ray_march(v, tile, iterations, steps, refine, bounds, ox, oy, oz, d.x, d.y, d.z, cam.c[12], cam.c[13]);
    water_pixel<MODE, SKY>(v, tile, iterations, mt, ox, oy, oz, d.x, d.y, d.z, m, k, out, sk, sun_size);
}

template <int MODE, bool TILED>
__global__ __launch_bounds__(256) void k_camera(DevView v, int tile, int iterations, int steps, int refine,
                                                const float* __restrict__ bounds, CameraRays cam, CameraMaterial mt,
                                                int width, int height, float* __restrict__ out) {
    camera_pixel<MODE, TILED, false>(v, tile, iterations, steps, refine, bounds, cam, mt, width, height, out, LutView{}, 0.0f);
}

template <bool TILED>
__global__ __launch_bounds__(256) void k_camera_sky(DevView v, int tile, int iterations, int steps, int refine,
                                                    const float* __restrict__ bounds, CameraRays cam, CameraMaterial mt,
                                                    LutView sk, float sun_size, int width, int height,
                                                    float* __restrict__ out) {
    camera_pixel<OCEAN_CAMERA_COLOR, TILED, true>(v, tile, iterations, steps, refine, bounds, cam, mt, width, height, out, sk,
                                                  sun_size);
}

// ---------------------------------------------------------------------------------------------------------------
// Camera views that see the bodies (ocean_camera_bodies*).  include/ocean/ocean.h has the definition: per pixel the
// slab test of the ray against every body's box, the nearest body met, and the nearer of that body and the water.
// The definition is a loop over all bodies per pixel; the kernel gets the same bits from fewer tests and samples.
//
// Cull per workgroup.  A workgroup is a 16 x 16 pixel tile (always the tiled mapping).  The bodies go by in chunks
// of 256; lane l of the workgroup forms what the slab test needs of body base + l that does not depend on the
// pixel (ob, l, h: the statements of ocean.h, so the same bits for every pixel) and tests the body's bounding
// sphere against a cone around the tile's rays and against [t0, t1].  The survivors are compacted into LDS in
// ascending b (a ballot per wave, then a prefix over the four waves' counts), and after a barrier every lane runs
// the slab test over them.  Survivors in ascending b and a strict `te <` keep the lowest b on ties, as the
// definition does.  OCEAN_CAMERA_CULL=0 makes every body a survivor.
//
// The cull is conservative: a body it drops is met by no ray of the tile.  In exact arithmetic:
//   - the cone.  The raw directions of a tile's pixels are affine in (i, j): they lie in the parallelogram of the
//     four corner pixels' raw directions.  The directions within an angle theta < 90 degrees of an axis form a convex
//     cone, so if the corners are within theta of the axis, every pixel is.  The axis a is the direction through the
//     tile's centre; sin(theta) is the largest |corner x a| and cos(theta) the smallest dot(corner, a) (a partial
//     tile uses the full tile's corners: a superset).  A tile with cos(theta) < 1/2 is not culled at all;
//   - the sphere.  With q near unit the slab test's box is c + A B, B the scaled box, A = P + Q / sigma, where P
//     projects on u, Q turns the plane across u and sigma^2 = 1 + 4 |u|^2 e, e = |q|^2 - 1; rot(u, qw, .) is
//     P + sigma Q.  For |e| <= 2^-10: 1 / sigma <= 1 + 2^-8 and |1 / sigma - sigma| <= 2^-7, so every point of the
//     box lies within hd (1 + 2^-8) + 2^-7 |bc| of ctr = c + rot(u, qw, bc), bc the scaled box's centre and hd half
//     its diagonal.  A body whose |q|^2 is further from 1 is a survivor: its box may be anything;
//   - the test.  With v = ctr - o, x = dot(v, a), y = |v x a|, a point at distance y cos(theta) - x sin(theta) or
//     more from every point of the solid cone (behind the apex the true distance, |v|, is larger still), so a body
//     with y cos(theta) - x sin(theta) > rad is off every ray, and one with |v| - rad > t1 or |v| + rad < t0 is
//     met outside [t0, t1] only.
// In fp32, with u = 2^-24, every length below is at most S = |v|_1 + |bc|_1 + hd (1-norms: larger than the 2-norms):
//   - the slab test itself reports `met` only for a ray that passes within 64 u S of the exact box: ob and db carry
//     at most 16 u |w| and 16 u from rot's four levels of operations, l and h one rounding each, n_i and f_i two;
//     one axis has |db_i| >= 1 / 2, which bounds tn and tf by 2 S, so the overlap tn <= tf can be wrong by 8 u S of
//     ray length, and the perturbed ob and db move the ray by 16 u |w| + 32 u S;
//   - the pixels' fp32 directions are within 8 u of the exact ones, and of unit length within 4 u: 12 u |v| across
//     and along the ray;
//   - v, a, the two products x and y (a cross product, not a difference of squares), cos and sin each carry at most
//     24 u S, 4 u, 24 u S, 8 u: the left side is off by at most 80 u S.
// Together less than 160 u S; the margin is 2^-16 S = 256 u S, added to rad.  Every compare is written so that a
// NaN makes a survivor.
//
// Stop the march at the body.  The body loop comes first, and the march runs with t_stop = te of the pixel's body
// (ray_march.h, STOP): a ray that reaches the body's distance above the water ends there.
struct alignas(16) BodySurvivor {  // 64 B: what the slab test reads of a body, and its index
    float obx, oby, obz, ux, uy, uz, qw, lx, ly, lz, hx, hy, hz;
    int b;
};
static_assert(sizeof(BodySurvivor) == 64, "four float4 per survivor");

// a rotated by the quaternion (u, w) (ocean.h, rot): t = 2 (u x a), (a + w t) + (u x t).
__device__ __forceinline__ Vec3 rotate(float ux, float uy, float uz, float w, float ax, float ay, float az) {
    const float tx = 2.0f * (uy * az - uz * ay), ty = 2.0f * (uz * ax - ux * az), tz = 2.0f * (ux * ay - uy * ax);
    Vec3 r;
    r.x = (ax + w * tx) + (uy * tz - uz * ty);
    r.y = (ay + w * ty) + (uz * tx - ux * tz);
    r.z = (az + w * tz) + (ux * ty - uy * tx);
    return r;
}

// One axis of the slab test: n_i and f_i, or false where the ray runs beside the slab.
__device__ __forceinline__ bool slab(float l, float h, float ob, float db, float& n, float& f) {
    if (db == 0.0f) {
        n = -__builtin_inff(), f = __builtin_inff();
        return fminf(l, h) <= ob && ob <= fmaxf(l, h);
    }
    const float a = (l - ob) / db, e = (h - ob) / db;
    n = fminf(a, e), f = fmaxf(a, e);
    return true;
}

constexpr float kCullMargin = 0x1p-16f;   // of S, above
constexpr float kUnitQuat = 0x1p-10f;     // |q|^2 within this of 1, above

// Record b of `bodies` as a survivor, but for ob: what the slab test reads of the body that does not depend on where
// the ray starts (l, h: the statements of ocean.h), and the body's origin c.
__device__ __forceinline__ BodySurvivor body_record(const float* __restrict__ bodies, int stride, int b, const BodyBox& box,
                                                    Vec3& c) {
    const float* B = bodies + (size_t)b * stride;
    const float sx = B[7], sy = B[8], sz = B[9];
    c.x = B[0], c.y = B[1], c.z = B[2];
    BodySurvivor sv = {};
    sv.ux = B[3], sv.uy = B[4], sv.uz = B[5], sv.qw = B[6];
    sv.lx = sx * box.b[0], sv.ly = sy * box.b[1], sv.lz = sz * box.b[2];
    sv.hx = sx * box.b[3], sv.hy = sy * box.b[4], sv.hz = sz * box.b[5];
    sv.b = b;
    return sv;
}

// The body's bounding sphere ("the sphere", above): r = ctr - c, its radius before the margin, |bc|_1 + hd for S, and
// whether |q|^2 is within kUnitQuat of 1 (false for a NaN: such a body is a survivor of every cull).
struct BodySphere {
    Vec3 r;
    float rad, size;
    bool unit;
};
__device__ __forceinline__ BodySphere body_sphere(const BodySurvivor& sv) {
    const float bx = 0.5f * (sv.lx + sv.hx), by = 0.5f * (sv.ly + sv.hy), bz = 0.5f * (sv.lz + sv.hz);
    const float ex = 0.5f * (sv.hx - sv.lx), ey = 0.5f * (sv.hy - sv.ly), ez = 0.5f * (sv.hz - sv.lz);
    const float hd = sqrtf((ex * ex + ey * ey) + ez * ez);
    const float bc1 = (fabsf(bx) + fabsf(by)) + fabsf(bz);
    const float qq = ((sv.ux * sv.ux + sv.uy * sv.uy) + sv.uz * sv.uz) + sv.qw * sv.qw;
    BodySphere sp;
    sp.r = rotate(sv.ux, sv.uy, sv.uz, sv.qw, bx, by, bz);
    sp.rad = hd * (1.0f + 0x1p-8f) + bc1 * 0x1p-7f;
    sp.size = bc1 + hd;
    sp.unit = fabsf(qq - 1.0f) <= kUnitQuat;
    return sp;
}

// The kept records of one chunk into s_body in ascending lane order, so in ascending b; their number.  Two barriers:
// every lane of the workgroup comes here, with w its wave and l its lane.
__device__ __forceinline__ int compact_survivors(bool keep, const BodySurvivor& sv, BodySurvivor* s_body, int* s_count,
                                                 int w, int l) {
    const unsigned long long mask = __ballot(keep);
    if (l == 0) s_count[w] = __popcll(mask);
    __syncthreads();  // the counts are there; every lane is done with the chunk before
    int first = 0, total = 0;
    for (int k = 0; k < 4; ++k) {
        const int n = s_count[k];
        first += k < w ? n : 0;
        total += n;
    }
    if (keep) s_body[first + __popcll(mask & ((1ull << l) - 1ull))] = sv;
    __syncthreads();  // the survivors are there
    return total;
}

// The slab test of ocean.h for one body: the ray from ob (in the body frame) along d (in the world's), met within
// [t0, t1] or not, and what the normal needs.
struct SlabMeet {
    bool met;
    float tn, nx, ny;
    Vec3 db;
};
__device__ __forceinline__ SlabMeet meet_box(const BodySurvivor& q, float obx, float oby, float obz, const Vec3& d,
                                             float t0, float t1) {
    SlabMeet m;
    m.db = rotate(-q.ux, -q.uy, -q.uz, q.qw, d.x, d.y, d.z);
    float nz, fx, fy, fz;
    bool met = slab(q.lx, q.hx, obx, m.db.x, m.nx, fx);
    met = slab(q.ly, q.hy, oby, m.db.y, m.ny, fy) && met;
    met = slab(q.lz, q.hz, obz, m.db.z, nz, fz) && met;
    m.tn = fmaxf(fmaxf(m.nx, m.ny), nz);
    const float tf = fminf(fminf(fx, fy), fz);
    m.met = met && m.tn <= tf && tf >= t0 && m.tn <= t1;
    return m;
}

// The nearest body met so far (ocean.h: the met body of smallest te, the lowest b on ties): b = -1 for none.
struct BodyMeet {
    int b;
    float te;
    Vec3 nw;
};
__device__ __forceinline__ BodyMeet no_body() { return BodyMeet{-1, __builtin_inff(), Vec3{0.0f, 0.0f, 0.0f}}; }

// Body q, tested as m says, against the nearest so far; the bodies come in ascending b, so the strict `te <` keeps
// the lowest b on ties.  The normal is formed for a new nearest body only.
__device__ __forceinline__ void keep_nearer(const BodySurvivor& q, const SlabMeet& m, const Vec3& d, float t0,
                                            BodyMeet& best) {
    const float te = fmaxf(m.tn, t0);
    if (m.met && te < best.te) {
        best.te = te;
        best.b = q.b;
        if (m.tn >= t0) {
            const bool on_x = m.nx == m.tn, on_y = !on_x && m.ny == m.tn;
            const float dbx = m.db.x, dby = m.db.y, dbz = m.db.z;  // values: a select of members is one of addresses
            const float dbi = on_x ? dbx : on_y ? dby : dbz;
            const float sign = dbi > 0.0f ? -1.0f : 1.0f;
            best.nw = rotate(q.ux, q.uy, q.uz, q.qw, on_x ? sign : 0.0f, on_y ? sign : 0.0f, on_x || on_y ? 0.0f : sign);
        } else {  // the ray starts inside the box
            best.nw.x = -d.x, best.nw.y = -d.y, best.nw.z = -d.z;
        }
    }
}

// paintc(nw) of ocean.h, the colour of a body's face with the world normal nw:
// A_c * (ka * amb(nw)_c + LC_c * fmaxf(dot(nw, L), 0)), amb the two-colour sky at nw.y or, with SKY, the table at nw.
template <bool SKY>
__device__ __forceinline__ void paint_colour(const CameraMaterial& mt, const BodyPaint& paint, const LutView& sk,
                                             const Vec3& nw, float* rgb) {
    float amb[3];
    if (SKY) {
        const float3 e = sky_lut(sk, nw.x, nw.y, nw.z);
        amb[0] = e.x, amb[1] = e.y, amb[2] = e.z;
    } else {
        for (int c = 0; c < 3; ++c) amb[c] = sky(mt.m[26 + c], mt.m[29 + c], nw.y);
    }
    const float lit = fmaxf(dot3(nw.x, nw.y, nw.z, mt.m[20], mt.m[21], mt.m[22]), 0.0f);
    for (int c = 0; c < 3; ++c) rgb[c] = paint.p[c] * (paint.p[3] * amb[c] + mt.m[23 + c] * lit);
}

// The body of the pixel whose ray from the eye runs along d, in the 16 x 16 tile at (i0, j0): the cull per chunk, the
// compaction and the slab tests of the comment above.  Every lane of the workgroup comes here (barriers inside).
__device__ __forceinline__ BodyMeet primary_body(const CameraRays& cam, const BodyBox& box,
                                                 const float* __restrict__ bodies, int stride, int count, int cull, int i0,
                                                 int j0, const Vec3& d, BodySurvivor* s_body, int* s_count) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const float ox = cam.c[0], oy = cam.c[1], oz = cam.c[2], t0 = cam.c[12], t1 = cam.c[13];

    // the tile's cone: axis, cos and sin of its half angle
    const Vec3 ax = pixel_direction(cam, (float)i0 + 7.5f, (float)j0 + 7.5f);
    float ct = 1.0f, st = 0.0f;
    for (int c = 0; c < 4; ++c) {
        const Vec3 e = pixel_direction(cam, (float)(i0 + 15 * (c & 1)), (float)(j0 + 15 * (c >> 1)));
        const float cx = e.y * ax.z - e.z * ax.y, cy = e.z * ax.x - e.x * ax.z, cz = e.x * ax.y - e.y * ax.x;
        ct = fminf(ct, dot3(e.x, e.y, e.z, ax.x, ax.y, ax.z));
        st = fmaxf(st, sqrtf((cx * cx + cy * cy) + cz * cz));
    }
    const bool culling = cull != 0 && ct >= 0.5f;

    // the pixel's body: the met body of smallest te, the lowest b on ties
    BodyMeet best = no_body();
    if (t1 < t0) return best;  // no body is met (uniform: before any barrier)
    for (int base = 0; base < count; base += 256) {
        const int b = base + (int)threadIdx.x;
        bool keep = false;
        BodySurvivor sv = {};
        if (b < count) {
            Vec3 c;
            sv = body_record(bodies, stride, b, box, c);
            const Vec3 ob = rotate(-sv.ux, -sv.uy, -sv.uz, sv.qw, ox - c.x, oy - c.y, oz - c.z);
            sv.obx = ob.x, sv.oby = ob.y, sv.obz = ob.z;
            keep = true;
            if (culling) {
                const BodySphere sp = body_sphere(sv);
                const float vx = (c.x - ox) + sp.r.x, vy = (c.y - oy) + sp.r.y, vz = (c.z - oz) + sp.r.z;
                const float S = ((fabsf(vx) + fabsf(vy)) + fabsf(vz)) + sp.size;
                const float rad = sp.rad + kCullMargin * S;
                const float x = dot3(vx, vy, vz, ax.x, ax.y, ax.z);
                const float px = vy * ax.z - vz * ax.y, py = vz * ax.x - vx * ax.z, pz = vx * ax.y - vy * ax.x;
                const float y = sqrtf((px * px + py * py) + pz * pz);
                const float dist = sqrtf((vx * vx + vy * vy) + vz * vz);
                const bool off = y * ct - x * st > rad || dist - rad > t1 || dist + rad < t0;
                keep = !(off && sp.unit);
            }
        }
        const int total = compact_survivors(keep, sv, s_body, s_count, w, l);
        for (int s = 0; s < total; ++s) {
            const BodySurvivor& q = s_body[s];  // one address for the wave: a broadcast
            keep_nearer(q, meet_box(q, q.obx, q.oby, q.obz, d, t0, t1), d, t0, best);
        }
    }
    return best;
}

// A body pixel of ocean_camera_bodies in MODE (element k of `out`).
template <int MODE, bool SKY>
__device__ __forceinline__ void body_pixel(const CameraMaterial& mt, const BodyPaint& paint, const LutView& sk,
                                           const BodyMeet& bm, size_t k, float* __restrict__ out) {
    if (MODE == OCEAN_CAMERA_RANGE) {
        out[k] = bm.te;
    } else if (MODE == OCEAN_CAMERA_HITS) {
        float4* o = reinterpret_cast<float4*>(out) + 2 * k;
        o[0] = make_float4(bm.te, 0.0f, 0.0f, (float)OCEAN_RAY_BODY);
        o[1] = make_float4(bm.nw.x, bm.nw.y, bm.nw.z, (float)bm.b);
    } else {
        float rgb[3];
        paint_colour<SKY>(mt, paint, sk, bm.nw, rgb);
        reinterpret_cast<float4*>(out)[k] = make_float4(rgb[0], rgb[1], rgb[2], (float)OCEAN_RAY_BODY);
    }
}

// Whether the pixel whose ray met the water as `m` says and the body `bm` is a body pixel (ocean.h: a body is met and
// the water is missed or met behind it; water wins ties, SUBMERGED stays).
__device__ __forceinline__ bool body_in_front(const BodyMeet& bm, const RayMeet& m) {
    return bm.b >= 0 && (m.status == OCEAN_RAY_BODY || m.status == OCEAN_RAY_MISS ||
                         (m.status == OCEAN_RAY_HIT && bm.te < m.t));
}

template <int MODE, bool SKY>
__global__ __launch_bounds__(256) void k_camera_bodies(DevView v, int tile, int iterations, int steps, int refine,
                                                       const float* __restrict__ bounds, CameraRays cam, CameraMaterial mt,
                                                       LutView sk, float sun_size, BodyBox box, BodyPaint paint,
                                                       const float* __restrict__ bodies, int stride, int count, int cull,
                                                       int width, int height, float* __restrict__ out) {
    __shared__ BodySurvivor s_body[256];
    __shared__ int s_count[4];
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    const int i = i0 + (w & 1) * 8 + (l & 7), j = j0 + (w >> 1) * 8 + (l >> 3);
    const Vec3 d = pixel_direction(cam, (float)i, (float)j);
    const float ox = cam.c[0], oy = cam.c[1], oz = cam.c[2], t0 = cam.c[12], t1 = cam.c[13];
    const BodyMeet bm = primary_body(cam, box, bodies, stride, count, cull, i0, j0, d, s_body, s_count);
    if (i >= width || j >= height) return;  // behind the last barrier
    const size_t k = (size_t)j * width + i;

    const RayMeet m = ray_march_until<true>(v, tile, iterations, steps, refine, bounds, ox, oy, oz, d.x, d.y, d.z, t0, t1,
                                            bm.b >= 0 ? bm.te : __builtin_nanf(""));
    if (body_in_front(bm, m))
        body_pixel<MODE, SKY>(mt, paint, sk, bm, k, out);
    else
        water_pixel<MODE, SKY>(v, tile, iterations, mt, ox, oy, oz, d.x, d.y, d.z, m, k, out, sk, sun_size);
}

// ---------------------------------------------------------------------------------------------------------------
// Camera views in which the water sees the bodies (ocean_camera_scene*).  include/ocean/ocean.h has the definition:
// ocean_camera_bodies' image, and at a water pixel the three places where the fragment stage of Water.shader reads
// scene geometry: the body behind the surface, fogged by its distance behind it; the shadow ray from the point met
// towards the sun; the mirror ray.  Again the definition tries every body for every ray, and the kernel gets the same
// bits from fewer tests.
//
// Order.  The primary body loop and the stopped march are k_camera_bodies'.  Then the pixel's fixed point and sample,
// which the mirror ray needs for n.  Body, MISS and SUBMERGED pixels are stored there, and their lanes, like those
// outside the image, stay alive to every barrier behind.  Then the second cull, the secondary rays, the shading.
//
// The second cull.  The secondary rays do not start at the eye, so the cone does not serve.  They start at the q of
// the workgroup's water pixels: the workgroup reduces the bounding box of those q (a butterfly per wave, then LDS
// across the four waves; a tile without a water pixel skips the stage uniformly), and with pc the box's centre, pr
// half its diagonal and rl the longest secondary ray, a body with |ctr - pc| > rad + pr + rl is further than rad from
// every point of every secondary ray of the tile.  ctr, rad and the unit-quaternion rule are those of the cull above.
// In exact arithmetic a ray's points are q + s r, s in [0, reach], so rl = reach max(|L|, |rd|); |rd|^2 = |V|^2 +
// 4 ndv^2 (|n|^2 - 1) is within 2^-20 of 1 for the fp32 unit vectors n and V, and rl = reach max(|L|, 1) (1 + 2^-10)
// covers both.  In fp32, with u = 2^-24 and every length at most S = |ctr - pc|_1 + |bc|_1 + hd + pr + rl:
//   - the slab test reports `met` only for a ray that passes within 64 u S of the exact box, and only for a part of
//     it within 8 u S of [0, reach] (the derivation above, with w = q - c, |w| <= |ctr - pc| + pr + |bc| (1 + 2^-7));
//   - the box is reduced from the very q the rays start at (fminf and fmaxf are exact); pc carries one rounding, and
//     the half extents are formed from the rounded pc as fmaxf(hi - pc, pc - lo), so that [pc - e, pc + e] holds the
//     box to one rounding of e; pr carries four more: 6 u S;
//   - ctr - pc is (c - pc) + r: 2 u S and rot's 16 u |bc|; its length 3 u S; the right side's sums 4 u S, rl's
//     products 3 u S.
// Together less than 110 u S; the margin is the 2^-16 S = 256 u S of the cull above.  Every compare is written so
// that a NaN makes a survivor.  The survivors' records carry c where the primary ones carry ob: a lane forms ob
// from its own q (the statements of ocean.h: w = q - c, ob = rot(-u, qw, w)), once for both rays.
//
// Registers and LDS: 73 VGPRs in LINKS mode and 95 in the two colour modes, no scratch; 16 KiB of survivors, 16 B of
// counts and 96 B of boxes.  At 95 VGPRs five waves per SIMD are resident, five workgroups per CU, and their 81 KiB
// of LDS fit the CU's 160 KiB: as for k_camera_bodies, the registers bound the occupancy, not the LDS.
template <int MODE, bool SKY>
__global__ __launch_bounds__(256) void k_camera_scene(DevView v, int tile, int iterations, int steps, int refine,
                                                      const float* __restrict__ bounds, CameraRays cam, CameraMaterial mt,
                                                      LutView sk, float sun_size, BodyBox box, BodyPaint paint,
                                                      SceneOptics op, const float* __restrict__ bodies, int stride,
                                                      int count, int cull, int width, int height,
                                                      float* __restrict__ out) {
    __shared__ BodySurvivor s_body[256];
    __shared__ int s_count[4];
    __shared__ float s_box[4][6];
    constexpr bool kLinks = MODE == OCEAN_CAMERA_LINKS;
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int i0 = blockIdx.x * 16, j0 = blockIdx.y * 16;
    const int i = i0 + (w & 1) * 8 + (l & 7), j = j0 + (w >> 1) * 8 + (l >> 3);
    const Vec3 d = pixel_direction(cam, (float)i, (float)j);
    const float ox = cam.c[0], oy = cam.c[1], oz = cam.c[2], t0 = cam.c[12], t1 = cam.c[13];
    const BodyMeet b1 = primary_body(cam, box, bodies, stride, count, cull, i0, j0, d, s_body, s_count);
    const bool inside = i < width && j < height;
    const size_t k = (size_t)j * width + i;  // used by the lanes inside only

    // the water on the ray, and every pixel that is not a water HIT pixel
    bool water = false;
    float tstar = 0.0f;
    if (inside) {
        const RayMeet m = ray_march_until<true>(v, tile, iterations, steps, refine, bounds, ox, oy, oz, d.x, d.y, d.z, t0,
                                                t1, b1.b >= 0 ? b1.te : __builtin_nanf(""));
        const bool body = body_in_front(b1, m);
        water = !body && m.status == OCEAN_RAY_HIT;
        tstar = m.t;
        if (kLinks) {
            if (!water)
                reinterpret_cast<float4*>(out)[k] = make_float4(1.0f, body ? (float)b1.b : -1.0f, -1.0f,
                                                                (float)(body ? OCEAN_RAY_BODY : m.status));
        } else if (body) {
            body_pixel<OCEAN_CAMERA_COLOR, SKY>(mt, paint, sk, b1, k, out);
        } else if (!water) {
            water_pixel<OCEAN_CAMERA_COLOR, SKY>(v, tile, iterations, mt, ox, oy, oz, d.x, d.y, d.z, m, k, out, sk, sun_size);
        }
    }

    // the point met, its normal, wave height and foam: the statements of water_pixel's colour mode
    float qx = 0.0f, qy = 0.0f, qz = 0.0f, nx = 0.0f, ny = 1.0f, nz = 0.0f, eta = 0.0f, foam = 0.0f;
    Vec3 rd = {0.0f, 1.0f, 0.0f};
    if (water) {
        qx = ox + tstar * d.x, qy = oy + tstar * d.y, qz = oz + tstar * d.z;
        const float2 p = surface_fixed_point(v, tile, qx, qz, iterations);
        const WorldSample s = sample_cascades(v, tile, p.x, p.y, tstar * mt.m[7]);
        const float4 n = normal_from_deriv(s.deriv.x, s.deriv.y, s.deriv.z, s.deriv.w);  // (0, 1, 0) without DERIV
        nx = n.x, ny = n.y, nz = n.z, eta = s.disp.y, foam = s.turb;
        const float vx = -d.x, vy = -d.y, vz = -d.z;
        const float ndv = dot3(nx, ny, nz, vx, vy, vz);
        rd.x = (2.0f * ndv) * nx - vx, rd.y = (2.0f * ndv) * ny - vy, rd.z = (2.0f * ndv) * nz - vz;
    }

    // the secondary rays: the shadow ray any-hit, the mirror ray nearest-hit
    const float reach = op.o[5];
    const Vec3 L = {mt.m[20], mt.m[21], mt.m[22]};
    const bool sun_up = L.y > 0.0f;
    bool shadowed = false;
    BodyMeet b2 = no_body();
    if (count > 0) {
        // the box of the workgroup's q: lanes that are no water pixel contribute nothing
        const float inf = __builtin_inff();
        float bb[6] = {water ? qx : inf, water ? qy : inf, water ? qz : inf, water ? qx : -inf, water ? qy : -inf,
                       water ? qz : -inf};
        for (int step = 1; step < 64; step <<= 1)
            for (int c = 0; c < 3; ++c) {
                bb[c] = fminf(bb[c], __shfl_xor(bb[c], step));
                bb[3 + c] = fmaxf(bb[3 + c], __shfl_xor(bb[3 + c], step));
            }
        if (l == 0)
            for (int c = 0; c < 6; ++c) s_box[w][c] = bb[c];
        __syncthreads();
        for (int c = 0; c < 3; ++c) {
            bb[c] = fminf(fminf(s_box[0][c], s_box[1][c]), fminf(s_box[2][c], s_box[3][c]));
            bb[3 + c] = fmaxf(fmaxf(s_box[0][3 + c], s_box[1][3 + c]), fmaxf(s_box[2][3 + c], s_box[3][3 + c]));
        }
        if (bb[0] <= bb[3]) {  // uniform: some lane is a water pixel
            const float pcx = 0.5f * (bb[0] + bb[3]), pcy = 0.5f * (bb[1] + bb[4]), pcz = 0.5f * (bb[2] + bb[5]);
            const float ex = fmaxf(bb[3] - pcx, pcx - bb[0]), ey = fmaxf(bb[4] - pcy, pcy - bb[1]);
            const float ez = fmaxf(bb[5] - pcz, pcz - bb[2]);
            const float pr = sqrtf((ex * ex + ey * ey) + ez * ez);
            const float rl = (reach * fmaxf(sqrtf((L.x * L.x + L.y * L.y) + L.z * L.z), 1.0f)) * (1.0f + 0x1p-10f);
            for (int base = 0; base < count; base += 256) {
                const int b = base + (int)threadIdx.x;
                bool keep = false;
                BodySurvivor sv = {};
                if (b < count) {
                    Vec3 c;
                    sv = body_record(bodies, stride, b, box, c);
                    sv.obx = c.x, sv.oby = c.y, sv.obz = c.z;  // c in ob's place: ob depends on the lane's q
                    keep = true;
                    if (cull != 0) {
                        const BodySphere sp = body_sphere(sv);
                        const float vx = (c.x - pcx) + sp.r.x, vy = (c.y - pcy) + sp.r.y, vz = (c.z - pcz) + sp.r.z;
                        const float S = ((((fabsf(vx) + fabsf(vy)) + fabsf(vz)) + sp.size) + pr) + rl;
                        const float dist = sqrtf((vx * vx + vy * vy) + vz * vz);
                        const bool off = dist > ((sp.rad + pr) + rl) + kCullMargin * S;
                        keep = !(off && sp.unit);
                    }
                }
                const int total = compact_survivors(keep, sv, s_body, s_count, w, l);
                if (water)
                    for (int s = 0; s < total; ++s) {
                        const BodySurvivor& q = s_body[s];  // one address for the wave: a broadcast
                        const Vec3 ob = rotate(-q.ux, -q.uy, -q.uz, q.qw, qx - q.obx, qy - q.oby, qz - q.obz);
                        if (sun_up && !shadowed) shadowed = meet_box(q, ob.x, ob.y, ob.z, L, 0.0f, reach).met;
                        keep_nearer(q, meet_box(q, ob.x, ob.y, ob.z, rd, 0.0f, reach), rd, 0.0f, b2);
                    }
            }
        }
    }
    if (!water) return;  // behind the last barrier

    if (kLinks) {
        reinterpret_cast<float4*>(out)[k] =
            make_float4(shadowed ? 0.0f : 1.0f, (float)b1.b, (float)b2.b, (float)OCEAN_RAY_HIT);
        return;
    }
    SceneTerms sc = {};
    sc.through = b1.b >= 0, sc.mirrored = b2.b >= 0, sc.shadowed = shadowed;
    if (sc.through) {
        sc.fog = exp2f(-(op.o[4] * (b1.te - tstar)));
        paint_colour<SKY>(mt, paint, sk, b1.nw, sc.seen);
    }
    if (sc.mirrored) paint_colour<SKY>(mt, paint, sk, b2.nw, sc.mirror);
    sc.sh[0] = op.o[0], sc.sh[1] = op.o[1], sc.sh[2] = op.o[2], sc.si = op.o[3];
    const float3 c = shade_hit<SKY, true>(mt, d.x, d.y, d.z, nx, ny, nz, eta, foam, v.deriv != nullptr, sk, sc);
    reinterpret_cast<float4*>(out)[k] = make_float4(c.x, c.y, c.z, (float)OCEAN_RAY_HIT);
}

// The launch grid of camera_pixel's two mappings: 16 x 16 pixel tiles, or 256 consecutive pixels per workgroup.
dim3 camera_groups(int width, int height, bool tiled) {
    if (tiled) return dim3((width + 15) / 16, (height + 15) / 16);
    return dim3((unsigned)(((size_t)width * height + 255) / 256));
}

}  // namespace

hipError_t launch_camera(const DevView& v, int tile, int mode, int iterations, int steps, int refine, const float* bounds,
                         const CameraRays& cam, const CameraMaterial& mt, int width, int height, bool tiled, float* out,
                         hipStream_t s) {
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)OCEAN_CAMERA_MAX_PIXELS) return hipErrorInvalidValue;
    const bool known = with_constant<OCEAN_CAMERA_HITS, OCEAN_CAMERA_RANGE, OCEAN_CAMERA_COLOR>(mode, [&](auto m) {
        (void)with_constant<0, 1>(tiled, [&](auto t) {  // a bool: one of the two matches
            launch(k_camera<decltype(m)::value, decltype(t)::value != 0>, camera_groups(width, height, tiled), dim3(256), 0,
                   s, v, tile, iterations, steps, refine, bounds, cam, mt, width, height, out);
        });
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_camera_sky(const DevView& v, int tile, int iterations, int steps, int refine, const float* bounds,
                             const CameraRays& cam, const CameraMaterial& mt, const LutView& sky, float sun_size, int width,
                             int height, bool tiled, float* out, hipStream_t s) {
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)OCEAN_CAMERA_MAX_PIXELS) return hipErrorInvalidValue;
    if (!sky.texels || sky.w < 2 || sky.h < 2) return hipErrorInvalidValue;
    (void)with_constant<0, 1>(tiled, [&](auto t) {  // a bool: one of the two matches
        launch(k_camera_sky<decltype(t)::value != 0>, camera_groups(width, height, tiled), dim3(256), 0, s, v, tile,
               iterations, steps, refine, bounds, cam, mt, sky, sun_size, width, height, out);
    });
    return hipGetLastError();
}

hipError_t launch_camera_bodies(const DevView& v, int tile, int mode, int iterations, int steps, int refine,
                                const float* bounds, const CameraRays& cam, const CameraMaterial& mt, const LutView& sky,
                                float sun_size, const BodyBox& box, const BodyPaint& paint, const float* bodies, int stride,
                                int count, bool cull, int width, int height, float* out, hipStream_t s) {
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)OCEAN_CAMERA_MAX_PIXELS) return hipErrorInvalidValue;
    if (stride < 10 || count < 0 || (count > 0 && !bodies)) return hipErrorInvalidValue;
    constexpr int kSky = OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT;
    if (mode == kSky && (!sky.texels || sky.w < 2 || sky.h < 2)) return hipErrorInvalidValue;
    const bool known = with_constant<OCEAN_CAMERA_HITS, OCEAN_CAMERA_RANGE, OCEAN_CAMERA_COLOR, kSky>(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        launch(k_camera_bodies<M & ~OCEAN_CAMERA_SKY_LUT, M == kSky>, camera_groups(width, height, true), dim3(256), 0, s, v,
               tile, iterations, steps, refine, bounds, cam, mt, sky, sun_size, box, paint, bodies, stride, count,
               cull ? 1 : 0, width, height, out);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

hipError_t launch_camera_scene(const DevView& v, int tile, int mode, int iterations, int steps, int refine,
                               const float* bounds, const CameraRays& cam, const CameraMaterial& mt, const LutView& sky,
                               float sun_size, const BodyBox& box, const BodyPaint& paint, const SceneOptics& optics,
                               const float* bodies, int stride, int count, bool cull, int width, int height, float* out,
                               hipStream_t s) {
    if (width < 1 || height < 1 || (size_t)width * height > (size_t)OCEAN_CAMERA_MAX_PIXELS) return hipErrorInvalidValue;
    if (stride < 10 || count < 0 || (count > 0 && !bodies)) return hipErrorInvalidValue;
    constexpr int kSky = OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT;
    if (mode == kSky && (!sky.texels || sky.w < 2 || sky.h < 2)) return hipErrorInvalidValue;
    const bool known = with_constant<OCEAN_CAMERA_COLOR, kSky, OCEAN_CAMERA_LINKS>(mode, [&](auto m) {
        constexpr int M = decltype(m)::value;
        launch(k_camera_scene<M & ~OCEAN_CAMERA_SKY_LUT, M == kSky>, camera_groups(width, height, true), dim3(256), 0, s, v,
               tile, iterations, steps, refine, bounds, cam, mt, sky, sun_size, box, paint, optics, bodies, stride, count,
               cull ? 1 : 0, width, height, out);
    });
    return known ? hipGetLastError() : hipErrorInvalidValue;
}

}  // namespace ocean
