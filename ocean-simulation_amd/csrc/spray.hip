// Spray particles (ocean_spray_step*): ballistic particles that are spawned from a whitecap list, advanced through
// substeps against the frame's water and retired where they fall back into the sea or outlive `life`, the
// survivors compacted into a pool in candidate order.  include/ocean/ocean.h has the definition.  Without this
// entry a host lands the emitter list, integrates on the CPU, uploads positions, queries the surface, lands the
// answers and compacts, every substep: the loop ocean_body_step removed for hulls.
//
// Candidates j = 0 .. M - 1, M = n + e known only on the device (the two headers are read there, clamped to the
// capacities the host passed), so the launch grid follows capacity + emit_capacity and lanes at or beyond M
// contribute nothing.  The compaction is the one compact.h describes, the predicate being `alive`:
//
//   step   the count launch.  A lane loads its candidate (two 16-B loads: a pool record, or an emitter record turned
//          into a fresh particle), takes up to S substeps, stopping at the first it does not survive, and stores the
//          stepped record to the context's scratch (the compaction's payload, 32 B per candidate) if it is still
//          alive.  The surface height under a particle is OCEAN_QUERY_SURFACE's, from surface_fixed_point /
//          sample_disp of sample_filter.h: the bits ocean_query_surface gives for that point.  The workgroup of item
//          0 leaves M beside the counts.
//   scan   the header's third field is read from that M.
//   emit   a survivor with rank < capacity copies its record from scratch to record 1 + rank.
//
// Air skip (ray_march.h has H and its proof): a particle with p'.y > H over a finite (p'.x, p'.z) is above every
// wave, so the first clause of `alive` is true without a sample (over a NaN or infinite x or z the height is a NaN,
// which retires the particle, so such a particle is sampled).  Only the outcome of the compare is used, so every result bit is the same with
// and without the bound; the number of samples is not.  A particle whose age has run out, or whose height is a
// NaN, is retired by the other clause or by the compare itself, and is not sampled either.
//
// A gather through L1 / L2 / Infinity Cache, K + 1 dependent round trips per substep below H: latency bound, no
// roofline claimed.  No inline assembly.
#include "compact.h"
#include "ocean_internal.h"
#include "ray_march.h"
#include "sample_filter.h"

namespace ocean {
namespace {

__global__ __launch_bounds__(kChunkThreads) void k_spray_step(DevView v, int tile, int iterations, int substeps,
                                                              SprayParams sp, const float* __restrict__ bounds,
                                                              const float4* __restrict__ pool, unsigned capacity,
                                                              const float4* __restrict__ emitters,
                                                              unsigned emit_capacity, unsigned items,
                                                              float4* __restrict__ stepped,
                                                              unsigned long long* __restrict__ masks,
                                                              unsigned* __restrict__ counts,
                                                              unsigned* __restrict__ total) {
    // the headers' W fields, clamped: the guard against a header this library did not write
    const unsigned n = min(__float_as_uint(pool[0].y), capacity);
    const unsigned e = emitters ? min(__float_as_uint(emitters[0].y), emit_capacity) : 0u;
    const unsigned m = n + e;
    const float h = sp.p[0], g = sp.p[1], kd = sp.p[2], wx = sp.p[3], wy = sp.p[4], wz = sp.p[5], life = sp.p[6];
    const float jet = sp.p[7], lift = sp.p[8];
    const bool skip = bounds != nullptr;
    const float H = skip ? air_height(bounds, v.C) : 0.0f;
    unsigned turn = 0;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned j = item * kChunkThreads + threadIdx.x;
        bool alive = false;
        if (j < m) {
            float px, py, pz, a, vx, vy, vz, tag;
            if (j < n) {
                const float4 r0 = pool[2 * (size_t)(1 + j)], r1 = pool[2 * (size_t)(1 + j) + 1];
                px = r0.x, py = r0.y, pz = r0.z, a = r0.w;
                vx = r1.x, vy = r1.y, vz = r1.z, tag = r1.w;
            } else {
                const size_t k = 1 + (size_t)(j - n);
                const float4 r0 = emitters[2 * k], r1 = emitters[2 * k + 1];
                px = r0.x, py = r0.y, pz = r0.z, a = 0.0f;
                vx = jet * r1.x, vy = jet * r1.y + lift * r0.w, vz = jet * r1.z;
                tag = r1.w;
            }
            alive = true;
            for (int s = 0; s < substeps && alive; ++s) {
                const float ax = kd * (wx - vx), ay = kd * (wy - vy) - g, az = kd * (wz - vz);
                vx = vx + h * ax, vy = vy + h * ay, vz = vz + h * az;
                px = px + h * vx, py = py + h * vy, pz = pz + h * vz;
                a = a + h;
                alive = a < life && py == py;  // decided without the water: the age, and a NaN fails py > eta
                // (H bounds the height over a finite point; over a NaN or infinite x or z the height is a NaN)
                if (alive && !(skip && py > H && fabsf(px) < INFINITY && fabsf(pz) < INFINITY)) {
                    const float2 p = surface_fixed_point(v, tile, px, pz, iterations);
                    alive = py > sample_disp(v, tile, p.x, p.y).y;  // rec[0]: sample_disp is sample_cascades' DISP
                }
            }
            if (alive) {
                stepped[2 * (size_t)j] = make_float4(px, py, pz, a);
                stepped[2 * (size_t)j + 1] = make_float4(vx, vy, vz, tag);
            }
        }
        compact_count(alive, item, turn, masks, counts);
        if (threadIdx.x == 0 && item == 0) *total = m;
    }
}

__global__ __launch_bounds__(kChunkThreads) void k_spray_emit(unsigned items, unsigned capacity,
                                                              const unsigned long long* __restrict__ masks,
                                                              const unsigned* __restrict__ offsets,
                                                              const float4* __restrict__ stepped,
                                                              float4* __restrict__ records) {
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        unsigned rank;
        bool done;
        if (!compact_rank(item, offsets, masks, capacity, rank, done)) {
            if (done) break;
            continue;
        }
        const size_t j = (size_t)item * kChunkThreads + threadIdx.x;
        float4* o = records + 2 * (size_t)rank;
        o[0] = stepped[2 * j];
        o[1] = stepped[2 * j + 1];
    }
}

// The chunks and the scratch of a call: the stepped records (32 B per candidate), the masks, the counts, M.
unsigned spray_items(int capacity, int emit_capacity) {
    return (unsigned)(((size_t)capacity + (size_t)emit_capacity + kChunkThreads - 1) / kChunkThreads);
}
CompactScratch spray_scratch(int capacity, int emit_capacity) {
    return compact_scratch(spray_items(capacity, emit_capacity), 32, true);
}

}  // namespace

size_t spray_scratch_bytes(int capacity, int emit_capacity) { return spray_scratch(capacity, emit_capacity).bytes; }

hipError_t launch_spray_step(const DevView& v, int tile, int iterations, int substeps, const SprayParams& sp,
                             const float* bounds, const float* pool, int capacity, const float* emitters,
                             int emit_capacity, void* scratch, float* out, hipStream_t s) {
    if (capacity <= 0 || emit_capacity < 0 || substeps <= 0 || (emitters == nullptr) != (emit_capacity == 0))
        return hipErrorInvalidValue;
    const unsigned items = spray_items(capacity, emit_capacity);
    const CompactScratch at = spray_scratch(capacity, emit_capacity);
    float4* stepped = scratch_at<float4>(scratch, at.payload);
    unsigned long long* masks = scratch_at<unsigned long long>(scratch, at.masks);
    unsigned* counts = scratch_at<unsigned>(scratch, at.counts);
    unsigned* total = scratch_at<unsigned>(scratch, at.total);
    const Items it{(int)items, v.max_groups};
    hipError_t e = launch_items(k_spray_step, kChunkThreads, it, s, v, tile, iterations, substeps, sp, bounds,
                                reinterpret_cast<const float4*>(pool), (unsigned)capacity,
                                reinterpret_cast<const float4*>(emitters), (unsigned)emit_capacity, items, stepped, masks,
                                counts, total);
    if (e != hipSuccess) return e;
    e = launch_compact_scan(counts, items, 0u, total, (unsigned)capacity, out, s);
    if (e != hipSuccess) return e;
    return launch_items(k_spray_emit, kChunkThreads, it, s, items, (unsigned)capacity, (const unsigned long long*)masks,
                        (const unsigned*)counts, (const float4*)stepped, reinterpret_cast<float4*>(out) + 2);
}

}  // namespace ocean
