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

// The colour of a hit pixel (ocean.h, "Colour of a hit"): the ray direction d, the normal n, the wave height and
// the foam at the point met.  has_foam: the context has DERIV and TURB (not DISPLACEMENT_ONLY).
// SKY: the sky is sky_lut over `sk`, else the two-colour sky of the material.
template <bool SKY>
__device__ __forceinline__ float3 shade_hit(const CameraMaterial& mt, float dx, float dy, float dz, float nx, float ny,
                                            float nz, float height, float foam, bool has_foam, const LutView& sk) {
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
    if (SKY) {  // all of -reflect(V, n)
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
        const float refr = m[c] + (coeff * m[12 + c]) * light;
        const float env = ((SKY ? env_sky[c] : sky(m[26 + c], m[29 + c], ry)) * kPi) * m[10];
        const float cook = sun_up ? ((light * dist) * geom) / ctden : 0.0f;
        const float ashk = sun_up ? light * as : 0.0f;
        const float refl = env + (cook + ashk * sndv) * m[11];
        float e = refr + fresnel * (refl - refr);
        if (foamy) e = e + m[19] * (m[16 + c] - e);
        out[c] = e;
    }
    return make_float3(out[0], out[1], out[2]);
}

// Pixel (i, j) -> element k = j * width + i of `out`.  TILED: a workgroup is a 16 x 16 pixel tile, wave w its
// 8 x 8 quadrant (w & 1, w >> 1), lane l the pixel (l & 7, l >> 3) of it; else 256 consecutive k per workgroup.
// SKY (colour mode only): the sky and the sun's disc of OCEAN_CAMERA_SKY_LUT over `sk`.
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

    const float fi = (float)i, fj = (float)j;
    const float rx = (cam.c[3] + fi * cam.c[6]) + fj * cam.c[9];
    const float ry = (cam.c[4] + fi * cam.c[7]) + fj * cam.c[10];
    const float rz = (cam.c[5] + fi * cam.c[8]) + fj * cam.c[11];
    const float len = sqrtf((rx * rx + ry * ry) + rz * rz);
    const float dx = rx / len, dy = ry / len, dz = rz / len;
    const float ox = cam.c[0], oy = cam.c[1], oz = cam.c[2];

    const RayMeet m = ray_march(v, tile, iterations, steps, refine, bounds, ox, oy, oz, dx, dy, dz, cam.c[12], cam.c[13]);
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

}  // namespace ocean
