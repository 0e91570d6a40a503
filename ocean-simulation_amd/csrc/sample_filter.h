// Texture filtering and the surface lookup shared by every point consumer of the finished textures (the
// world sampler, the surface and velocity queries, the surface grids and the buoyant bodies): the bilinear /
// trilinear taps of ocean_sample_world as include/ocean/ocean.h states them, the cascade sums built from
// them, and on top of those the surface query's fixed point, its residual and its record.  Device code
// only; every function is inlined into its kernel, so all kernels run the same fp32 operations in the same
// order (the build has -ffp-contract=off) and one numpy restatement checks them all bit for bit.
//   level texture of side m, uv = (x / L, z / L):  sx = u * m - 0.5, sy = v * m - 0.5;
//   i = floor(s), f = s - floor(s); texel columns i mod m, i + 1 mod m (Repeat), rows alike;
//   bilinear = lerp(lerp(t00, t10, fx), lerp(t01, t11, fx), fy), lerp(a, b, f) = a + f (b - a);
//   trilinear (DERIV, TURB with OCEAN_F_MIPS): lod clamped to [0, log2 N],
//   lerp(level floor(lod), level floor(lod) + 1, lod - floor(lod)); without mip chains
//   and for DISP, level 0.
#pragma once

#include "ocean_internal.h"
#include "spectrum_math.h"

namespace ocean {

struct Bil {
    int x0, x1, y0, y1;
    float fx, fy;
};

// Texel coordinates + weights of a bilinear tap at uv on an m x m level (m a power
// of two).  floor(s) is wrapped exactly in float (integers, power-of-two scaling),
// so any finite uv works without integer overflow.
__device__ __forceinline__ Bil bil(float u, float v, int m) {
    const float fm = (float)m, inv = 1.0f / fm;
    const float sx = u * fm - 0.5f, sy = v * fm - 0.5f;
    const float flx = floorf(sx), fly = floorf(sy);
    Bil b;
    b.fx = sx - flx;
    b.fy = sy - fly;
    const int ix = (int)(flx - fm * floorf(flx * inv)), iy = (int)(fly - fm * floorf(fly * inv));
    b.x0 = ix;
    b.x1 = (ix + 1) & (m - 1);
    b.y0 = iy;
    b.y1 = (iy + 1) & (m - 1);
    return b;
}

__device__ __forceinline__ float4 lerp4(float4 a, float4 b, float f) {
    return make_float4(a.x + f * (b.x - a.x), a.y + f * (b.y - a.y), a.z + f * (b.z - a.z), a.w + f * (b.w - a.w));
}

__device__ __forceinline__ float4 add4(float4 a, float4 b) {
    return make_float4(a.x + b.x, a.y + b.y, a.z + b.z, a.w + b.w);
}

__device__ __forceinline__ float4 tap(const float4* __restrict__ t, int m, const Bil& b) {
    const float4 t00 = t[(size_t)b.y0 * m + b.x0], t10 = t[(size_t)b.y0 * m + b.x1];
    const float4 t01 = t[(size_t)b.y1 * m + b.x0], t11 = t[(size_t)b.y1 * m + b.x1];
    return lerp4(lerp4(t00, t10, b.fx), lerp4(t01, t11, b.fx), b.fy);
}

// Level l of a slice: level 0 is the texture slice, levels >= 1 come from its mip chain.
__device__ __forceinline__ const float4* level_ptr(const float4* tex0, const float4* chain, size_t chain_len,
                                                   int slice, int n, int l) {
    if (l == 0) return tex0 + (size_t)slice * n * n;
    size_t off = 0;
    for (int k = 1; k < l; ++k) off += (size_t)(n >> k) * (n >> k);
    return chain + (size_t)slice * chain_len + off;
}

__device__ __forceinline__ float4 tri(const float4* tex0, const float4* chain, size_t chain_len, int slice, int n,
                                      int logn, float u, float v, float lod) {
    if (!chain || !(lod > 0.0f)) return tap(tex0 + (size_t)slice * n * n, n, bil(u, v, n));
    const float lc = fminf(lod, (float)logn);
    const int l0 = (int)floorf(lc), l1 = min(l0 + 1, logn);
    const float f = lc - (float)l0;
    const int m0 = n >> l0, m1 = n >> l1;
    const float4 a = tap(level_ptr(tex0, chain, chain_len, slice, n, l0), m0, bil(u, v, m0));
    const float4 b = tap(level_ptr(tex0, chain, chain_len, slice, n, l1), m1, bil(u, v, m1));
    return lerp4(a, b, f);
}

// The .x channel of tap / tri alone: the same texels, weights and operations on that channel, 4 B per texel.
__device__ __forceinline__ float tap_x(const float4* __restrict__ t, int m, const Bil& b) {
    const float t00 = t[(size_t)b.y0 * m + b.x0].x, t10 = t[(size_t)b.y0 * m + b.x1].x;
    const float t01 = t[(size_t)b.y1 * m + b.x0].x, t11 = t[(size_t)b.y1 * m + b.x1].x;
    const float a = t00 + b.fx * (t10 - t00), c = t01 + b.fx * (t11 - t01);
    return a + b.fy * (c - a);
}

__device__ __forceinline__ float tri_x(const float4* tex0, const float4* chain, size_t chain_len, int slice, int n,
                                       int logn, float u, float v, float lod) {
    if (!chain || !(lod > 0.0f)) return tap_x(tex0 + (size_t)slice * n * n, n, bil(u, v, n));
    const float lc = fminf(lod, (float)logn);
    const int l0 = (int)floorf(lc), l1 = min(l0 + 1, logn);
    const float f = lc - (float)l0;
    const int m0 = n >> l0, m1 = n >> l1;
    const float a = tap_x(level_ptr(tex0, chain, chain_len, slice, n, l0), m0, bil(u, v, m0));
    const float b = tap_x(level_ptr(tex0, chain, chain_len, slice, n, l1), m1, bil(u, v, m1));
    return a + f * (b - a);
}

// Deferred TURB (DevView::turb_foam): the float4 array is stale and the foam state is TURB's level 0, so tap_x's
// four texels come from the state, one slice of which is column-tile-major [N/W][N][W] (W = DevView::tile_w;
// spectrum.hip tiled_index): texel (y, x) sits at ((x / W) N + y) W + x % W.  The same values as TURB.x, the same
// weights and operations: bit-identical to tap_x on the materialised array.
__device__ __forceinline__ float tap_foam(const float* __restrict__ t, int n, int w, const Bil& b) {
    // W is a power of two (inter_w(N), or 4) and a slice has at most 2^24 texels: shifts and masks on 32-bit indices
    // (a division by a runtime W per tap measured 3-6 us on a 2^20-node whitecap count, docs/MEASUREMENTS.md section 33)
    const int sh = __ffs(w) - 1;
    auto at = [&](int y, int x) { return t[((((x >> sh) * n + y) << sh) | (x & (w - 1)))]; };
    const float t00 = at(b.y0, b.x0), t10 = at(b.y0, b.x1);
    const float t01 = at(b.y1, b.x0), t11 = at(b.y1, b.x1);
    const float a = t00 + b.fx * (t10 - t00), c = t01 + b.fx * (t11 - t01);
    return a + b.fy * (c - a);
}

// TURB.x of slice `slice` at (u, w, lod), tri_x's result bit for bit (and tri's .x: the same operations on that
// channel).  While the array is stale, level 0 is tapped from the foam state; levels >= 1 are the mip chain's
// (mips.hip boxes level 1 from the foam state in either mode) and l1 >= 1 always (N >= 16).
__device__ __forceinline__ float turb_x(const DevView& v, int slice, float u, float w, float lod) {
    if (!v.turb_foam) return tri_x(v.turb, v.turb_mips, v.mip_chain, slice, v.n, v.logn, u, w, lod);
    const float* f0 = v.foam + (size_t)slice * v.n * v.n;
    if (!v.turb_mips || !(lod > 0.0f)) return tap_foam(f0, v.n, v.tile_w, bil(u, w, v.n));
    const float lc = fminf(lod, (float)v.logn);
    const int l0 = (int)floorf(lc), l1 = min(l0 + 1, v.logn);
    const float f = lc - (float)l0;
    const int m0 = v.n >> l0, m1 = v.n >> l1;
    const float a = l0 == 0 ? tap_foam(f0, v.n, v.tile_w, bil(u, w, m0))
                            : tap_x(level_ptr(v.turb, v.turb_mips, v.mip_chain, slice, v.n, l0), m0, bil(u, w, m0));
    const float b = tap_x(level_ptr(v.turb, v.turb_mips, v.mip_chain, slice, v.n, l1), m1, bil(u, w, m1));
    return a + f * (b - a);
}

// What Water.shader reads at world (x, z) of tile `tile`, summed over the cascades in order from 0:
// DISP at level 0, DERIV and 1 - saturate(TURB.x) at `lod` (zero on DISPLACEMENT_ONLY contexts).
struct WorldSample {
    float4 disp, deriv;
    float turb;
};

__device__ __forceinline__ WorldSample sample_cascades(const DevView& v, int tile, float x, float z, float lod) {
    WorldSample s;
    s.disp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s.deriv = s.disp;
    s.turb = 0.0f;
    for (int c = 0; c < v.C; ++c) {
        const float L = v.casc[c * 5];
        const float u = x / L, w = z / L;  // worldUV / _Wavelengths[i] (Water.shader:325, :341)
        const int slice = tile * v.C + c;
        s.disp = add4(s.disp, tap(v.disp + (size_t)slice * v.n * v.n, v.n, bil(u, w, v.n)));  // no mips (:325)
        if (v.deriv) {
            s.deriv = add4(s.deriv, tri(v.deriv, v.deriv_mips, v.mip_chain, slice, v.n, v.logn, u, w, lod));
            // (a stale array, deferred TURB: the same value from the foam state, turb_x)
            const float tb = v.turb_foam ? turb_x(v, slice, u, w, lod)
                                         : tri(v.turb, v.turb_mips, v.mip_chain, slice, v.n, v.logn, u, w, lod).x;
            s.turb = s.turb + (1.0f - fminf(fmaxf(tb, 0.0f), 1.0f));  // 1 - saturate(.x) (:343)
        }
    }
    return s;
}

// The DISP taps of sample_cascades alone: the same operations on the same texels, so the result is
// bit-identical to sample_cascades(...).disp.
__device__ __forceinline__ float4 sample_disp(const DevView& v, int tile, float x, float z) {
    float4 disp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int c = 0; c < v.C; ++c) {
        const float L = v.casc[c * 5];
        const float u = x / L, w = z / L;
        const int slice = tile * v.C + c;
        disp = add4(disp, tap(v.disp + (size_t)slice * v.n * v.n, v.n, bil(u, w, v.n)));
    }
    return disp;
}

// Vs(x, z) of ocean_query_velocity: the bilinear taps of VEL (level 0) summed over the cascades like DISP.
__device__ __forceinline__ float4 sample_velocity(const DevView& v, const float4* __restrict__ vel, int tile, float x,
                                                  float z) {
    float4 vs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    for (int c = 0; c < v.C; ++c) {
        const float L = v.casc[c * 5];
        const int slice = tile * v.C + c;
        vs = add4(vs, tap(vel + (size_t)slice * v.n * v.n, v.n, bil(x / L, z / L, v.n)));
    }
    return vs;
}

// The full sample at (x, z) with the VEL taps beside it: per cascade one Bil serves the DISP, DERIV and VEL texels.
// disp and deriv are sample_cascades(v, tile, x, z, 0)'s bit for bit (lod 0 is level 0 with and without mip
// chains), vs is sample_velocity's; TURB, which no body term reads, is not tapped.
__device__ __forceinline__ void sample_cascades_vel(const DevView& v, const float4* __restrict__ vel, int tile, float x,
                                                    float z, WorldSample& s, float4& vs) {
    s.disp = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    s.deriv = s.disp;
    s.turb = 0.0f;
    vs = s.disp;
    for (int c = 0; c < v.C; ++c) {
        const float L = v.casc[c * 5];
        const size_t slice = (size_t)(tile * v.C + c) * v.n * v.n;
        const Bil b = bil(x / L, z / L, v.n);
        s.disp = add4(s.disp, tap(v.disp + slice, v.n, b));
        if (v.deriv) s.deriv = add4(s.deriv, tap(v.deriv + slice, v.n, b));
        vs = add4(vs, tap(vel + slice, v.n, b));
    }
}

// The TURB taps of sample_cascades alone (a context with TURB: not DISPLACEMENT_ONLY): the same operations on
// the same texels, so the result is bit-identical to sample_cascades(...).turb, with mip chains and lod > 0 too.
__device__ __forceinline__ float sample_foam(const DevView& v, int tile, float x, float z, float lod) {
    float turb = 0.0f;
    for (int c = 0; c < v.C; ++c) {
        const float L = v.casc[c * 5];
        const float u = x / L, w = z / L;
        const float tb = turb_x(v, tile * v.C + c, u, w, lod);
        turb = turb + (1.0f - fminf(fmaxf(tb, 0.0f), 1.0f));
    }
    return turb;
}

// The surface above a world point q (OCEAN_QUERY_SURFACE, query.hip has the derivation): `iterations` steps
// of the fixed point p <- q - D_xz(p) from p = q.  Returns p = (px, pz).
__device__ __forceinline__ float2 surface_fixed_point(const DevView& v, int tile, float qx, float qz, int iterations) {
    float px = qx, pz = qz;
    for (int k = 0; k < iterations; ++k) {
        const float4 d = sample_disp(v, tile, px, pz);
        px = qx - d.x;
        pz = qz - d.z;
    }
    return make_float2(px, pz);
}

// r = |p + D_xz(p) - q|_inf for the displacement `disp` sampled at p: what the next step would have started from.
__device__ __forceinline__ float surface_residual(float4 disp, float2 p, float qx, float qz) {
    return fmaxf(fabsf((p.x + disp.x) - qx), fabsf((p.y + disp.z) - qz));
}

// The surface query's record of the full sample `s` taken at p: (height, p.x, p.z, residual), (normal, foam).
struct SurfaceRecord {
    float4 at, nf;
};

__device__ __forceinline__ SurfaceRecord surface_record(const WorldSample& s, float2 p, float qx, float qz) {
    const float r = surface_residual(s.disp, p, qx, qz);
    const float4 nrm = normal_from_deriv(s.deriv.x, s.deriv.y, s.deriv.z, s.deriv.w);  // (0, 1, 0) without DERIV
    SurfaceRecord rec;
    rec.at = make_float4(s.disp.y, p.x, p.y, r);
    rec.nf = make_float4(nrm.x, nrm.y, nrm.z, s.turb);
    return rec;
}

// Node (i, j) of a regular grid (ocean_surface_grid, ocean_whitecaps): (qx, qz), one fp32 multiply and one fp32
// add each (ocean.h).  I: int or unsigned, i and j below 2^22, so the conversion is exact either way.
template <class I>
__device__ __forceinline__ float2 grid_node(I i, I j, float x0, float z0, float dx, float dz) {
    return make_float2(x0 + (float)i * dx, z0 + (float)j * dz);
}

// GetWaterHeight's texel index (WaterBody.cs:195-209), OCEAN_QUERY_REFERENCE: InverseLerp(-N/2, N/2, .) is
// saturate((v - a) / (b - a)).
__device__ __forceinline__ int reference_texel(float w, int n) {
    const float a = (float)(-(n / 2)), b = (float)(n / 2);
    const float u = fminf(fmaxf((w - a) / (b - a), 0.0f), 1.0f);
    return min(max((int)(u * (float)n), 0), n - 1);
}

}  // namespace ocean
