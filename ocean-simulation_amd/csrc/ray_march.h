// The march of a ray against the ocean surface, shared by the ray casts (ray.hip) and the camera views
// (view.hip): both kernels run these statements, so a pixel's ray meets the water where ocean_raycast says the
// same ray does, bit for bit.  include/ocean/ocean.h has the definition: a fixed march over S + 1 nodes, B
// bisections of the first interval that crosses.  The height under a ray point is OCEAN_QUERY_SURFACE's, from
// the same inlined functions (sample_filter.h), so every node's f is the bits a host would get from
// ocean_query_surface for that point.  Device code only.
//
// A ray is a chain of dependent L2 / Infinity-Cache round trips, K + 1 per node: latency bound, hidden by
// occupancy alone.  Two things keep the chain short.
//
// One evaluation site.  The march and the bisection are one loop whose body evaluates f at "the next t" and
// then decides what the next t is.  The lanes of a wave that still march and those that already bisect issue
// the same taps together; two loops would run the phases one after the other, each with the lanes of the
// other masked off.
//
// Air skip.  A node above every wave has f > 0 without a sample, and only the sign of f is used at a node.  H
// bounds the height from above: with max_c and A_c = max(|min_c|, |max_c|) the bounds of DISP.y of cascade c
// (bounds.hip, exact) and u = 2^-24,
//   - lerp(a, b, f) = a + f (b - a) with f in [0, 1): the exact value lies between a and b; the three
//     roundings (b - a, the product, the sum) add at most (2 + 2 + 1) u A_c (1 + 2 u) when |a|, |b| <= A_c;
//   - a bilinear tap is two levels of lerps: its y is at most max_c + 11 u A_c;
//   - the cascade sum starts from +0 (the first add is exact) and rounds at most 4 more times, each by at
//     most u times the sum of the taps' magnitudes: 4 u (1 + 11 u) A, A = sum_c A_c.
// So height <= sum_c max_c + 16 u A, at any p: the fixed point moves p, not the bound, and H holds at any K.
// The kernels form H = fl(sum_c max_c) + 2^-19 fl(A) in fp32: the two sums lose at most 4 u A and 5 u A of
// relative size, the scaling by 2^-19 = 32 u is exact and the last add rounds by about u A, which leaves
// H >= sum_c max_c + 26 u A.  pos.y > H then gives pos.y > height and, fp32 subtraction being monotone with
// gradual underflow, f = pos.y - height > 0: the branch the sampled f would have taken.  The result does not
// depend on the bound, only the number of samples does.  (NaN texels or rays: unspecified numbers, as ocean.h
// says; bil() wraps every index whatever its input, and nothing here indexes by t.)
//
// Stop at a body (STOP, the camera views with bodies).  A caller that already knows an opaque thing on the ray at
// t_stop needs the water only in front of it.  A node t_j >= t_stop that is above the water, with no crossing
// before it, ends the march: a later crossing would be bracketed by a = t_(j'-1) >= t_j and b = t_j' > a, the
// bisection keeps a < b (a midpoint equal to a is above, as a is, and moves a, never b), so t* = b > t_stop, and a
// MISS has no t* at all; in both cases the thing at t_stop is what the ray meets first.  The march then reports
// OCEAN_RAY_BODY and no t*.  A node at or behind t_stop that is under the water bisects as usual, and the caller
// compares t* with t_stop.  HIT, MISS and SUBMERGED results are those of the full march, bit for bit; only the
// number of samples differs.  t_stop = NaN never stops (every compare with it is false).
#pragma once

#include "ocean_internal.h"
#include "sample_filter.h"

namespace ocean {

// H of the comment above from the tile's bounds records, float[C][8] (y: elements 1 and 5).
__device__ __forceinline__ float air_height(const float* __restrict__ bounds, int C) {
    float top = 0.0f, mag = 0.0f;
    for (int c = 0; c < C; ++c) {
        const float lo = bounds[8 * c + 1], hi = bounds[8 * c + 5];
        top = top + hi;
        mag = mag + fmaxf(fabsf(lo), fabsf(hi));
    }
    return top + mag * 0x1p-19f;
}

// Where the ray (o, d, t0, t1) meets the water: t* and the status (OCEAN_RAY_*).  bounds: the tile's records for
// the air skip, or null to sample every node.
struct RayMeet {
    float t;
    int status;
};

template <bool STOP>
__device__ __forceinline__ RayMeet ray_march_until(const DevView& v, int tile, int iterations, int steps, int refine,
                                                   const float* __restrict__ bounds, float ox, float oy, float oz,
                                                   float dx, float dy, float dz, float t0, float t1, float t_stop) {
    const bool skip = bounds != nullptr;
    const float H = skip ? air_height(bounds, v.C) : 0.0f;
    const float dt = (t1 - t0) / (float)steps;

    // node j of the march while !refining, then the bisection of [a, b] with `left` midpoints to go
    float t = t0, a = t0, b = t0;
    int j = 0, left = refine, status = OCEAN_RAY_MISS;
    bool refining = false;
    for (;;) {
        const float px = ox + t * dx, py = oy + t * dy, pz = oz + t * dz;
        bool above = skip && py > H;
        if (!above) {
            const float2 p = surface_fixed_point(v, tile, px, pz, iterations);
            above = py - sample_disp(v, tile, p.x, p.y).y > 0.0f;  // rec[0]: sample_disp is sample_cascades' DISP
        }
        if (!refining) {
            if (above) {
                if (STOP && t >= t_stop) {
                    status = OCEAN_RAY_BODY;
                    break;
                }
                if (j == steps) {
                    status = OCEAN_RAY_MISS;
                    break;
                }
                a = t;
                ++j;
                t = t0 + (float)j * dt;
                continue;
            }
            if (j == 0) {
                status = OCEAN_RAY_SUBMERGED;
                break;
            }
            b = t;  // a = t_(j-1), b = t_j
            refining = true;
        } else {
            if (above)
                a = t;
            else
                b = t;
            --left;
        }
        if (left == 0) {
            status = OCEAN_RAY_HIT;
            t = b;
            break;
        }
        t = 0.5f * (a + b);
    }
    RayMeet m;
    m.t = t;
    m.status = status;
    return m;
}

// The full march: ocean_raycast's and ocean_camera's.
__device__ __forceinline__ RayMeet ray_march(const DevView& v, int tile, int iterations, int steps, int refine,
                                             const float* __restrict__ bounds, float ox, float oy, float oz, float dx,
                                             float dy, float dz, float t0, float t1) {
    return ray_march_until<false>(v, tile, iterations, steps, refine, bounds, ox, oy, oz, dx, dy, dz, t0, t1, 0.0f);
}

}  // namespace ocean
