// Whitecap emitters (ocean_whitecaps*): the nodes of a regular grid whose foam reaches a threshold, compacted
// into a list in ascending node order.  Every other consumer answers "what is the water doing here?" for a
// place the host already knows; a spray, foam-particle or audio system asks where the sea is breaking, and
// without this entry it reads a TURB slice or a dense vertex grid back to threshold a few hundred emitters
// out of it.
//
// The grid is ocean_surface_grid's (grid_node of sample_filter.h), and node (i, j) is candidate k = j * nx + i of
// the compaction that compact.h describes.  Node k is selected iff foam(k) >= threshold, foam = sample_foam of
// sample_filter.h (the S(q)[3] of ocean_sample_world).
//
//   count  a lane reads the TURB taps of its node alone.
//   emit   only selected lanes with rank < capacity sample DISP, VEL and the foam and store their two float4.
//
// A gather through L1 / L2 / Infinity Cache like the grid kernel's: no roofline claimed.  No inline assembly.
#include "compact.h"
#include "ocean_internal.h"
#include "sample_filter.h"

namespace ocean {
namespace {

// Node k of the grid: (qx, qz).
__device__ __forceinline__ float2 node_at(unsigned k, unsigned nx, float x0, float z0, float dx, float dz) {
    const unsigned j = k / nx, i = k - j * nx;
    return grid_node(i, j, x0, z0, dx, dz);
}

__global__ __launch_bounds__(kChunkThreads) void k_whitecap_count(DevView v, int tile, float lod, float threshold,
                                                                  float x0, float z0, float dx, float dz, unsigned nx,
                                                                  unsigned nodes, unsigned items,
                                                                  unsigned long long* __restrict__ masks,
                                                                  unsigned* __restrict__ counts) {
    unsigned turn = 0;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        const unsigned k = item * kChunkThreads + threadIdx.x;
        bool sel = false;
        if (k < nodes) {
            const float2 q = node_at(k, nx, x0, z0, dx, dz);
            sel = sample_foam(v, tile, q.x, q.y, lod) >= threshold;  // false for a NaN foam
        }
        compact_count(sel, item, turn, masks, counts);
    }
}

__global__ __launch_bounds__(kChunkThreads) void k_whitecap_emit(DevView v, const float4* __restrict__ vel, int tile,
                                                                 float lod, float x0, float z0, float dx, float dz,
                                                                 unsigned nx, unsigned items, unsigned capacity,
                                                                 const unsigned long long* __restrict__ masks,
                                                                 const unsigned* __restrict__ offsets,
                                                                 float4* __restrict__ records) {
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        unsigned rank;
        bool done;
        if (!compact_rank(item, offsets, masks, capacity, rank, done)) {
            if (done) break;
            continue;
        }
        const unsigned k = item * kChunkThreads + threadIdx.x;
        const float2 q = node_at(k, nx, x0, z0, dx, dz);
        const float4 d = sample_disp(v, tile, q.x, q.y);
        float4 vs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (vel) vs = sample_velocity(v, vel, tile, q.x, q.y);  // ocean_query_velocity's Vs(q) with no fixed-point step
        float4* o = records + 2 * (size_t)rank;
        o[0] = make_float4(q.x + d.x, d.y, q.y + d.z, sample_foam(v, tile, q.x, q.y, lod));
        o[1] = make_float4(vs.x, vs.y, vs.z, (float)k);  // k < 2^22: exact
    }
}

// The context's scratch holds every grid: the masks, then the counts, of OCEAN_GRID_MAX_NODES nodes.
CompactScratch max_grid_scratch() { return compact_scratch(OCEAN_GRID_MAX_NODES / kChunkThreads, 0, false); }

}  // namespace

size_t whitecap_scratch_bytes() { return max_grid_scratch().bytes; }

hipError_t launch_whitecaps(const DevView& v, const float4* vel, int tile, float lod, float threshold, float x0, float z0,
                            float dx, float dz, int nx, int ny, int capacity, void* scratch, float* out, hipStream_t s) {
    if (nx <= 0 || ny <= 0 || capacity <= 0 || (uint64_t)nx * (uint64_t)ny > (uint64_t)OCEAN_GRID_MAX_NODES)
        return hipErrorInvalidValue;
    const unsigned nodes = (unsigned)nx * (unsigned)ny;
    const unsigned items = (nodes + kChunkThreads - 1) / kChunkThreads;
    const CompactScratch at = max_grid_scratch();
    unsigned long long* masks = scratch_at<unsigned long long>(scratch, at.masks);
    unsigned* counts = scratch_at<unsigned>(scratch, at.counts);
    const Items it{(int)items, v.max_groups};
    hipError_t e = launch_items(k_whitecap_count, kChunkThreads, it, s, v, tile, lod, threshold, x0, z0, dx, dz,
                                (unsigned)nx, nodes, items, masks, counts);
    if (e != hipSuccess) return e;
    e = launch_compact_scan(counts, items, nodes, nullptr, (unsigned)capacity, out, s);
    if (e != hipSuccess) return e;
    return launch_items(k_whitecap_emit, kChunkThreads, it, s, v, vel, tile, lod, x0, z0, dx, dz, (unsigned)nx, items,
                        (unsigned)capacity, (const unsigned long long*)masks, (const unsigned*)counts,
                        reinterpret_cast<float4*>(out) + 2);
}

}  // namespace ocean
