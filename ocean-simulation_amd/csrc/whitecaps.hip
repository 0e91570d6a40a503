// Whitecap emitters (ocean_whitecaps*): the nodes of a regular grid whose foam reaches a threshold, compacted
// into a list in ascending node order.  Every other consumer answers "what is the water doing here?" for a
// place the host already knows; a spray, foam-particle or audio system asks where the sea is breaking, and
// without this entry it reads a TURB slice or a dense vertex grid back to threshold a few hundred emitters
// out of it.
//
// The grid is ocean_surface_grid's: node (i, j) at qx = x0 + (float)i * dx, qz = z0 + (float)j * dz, index
// k = j * nx + i.  Node k is selected iff foam(k) >= threshold, foam = sample_foam of sample_filter.h (the
// S(q)[3] of ocean_sample_world), and writes record 1 + rank(k), rank(k) = the selected nodes below k, while
// rank(k) < capacity.  An order-preserving stream compaction in three launches, with no atomics and no
// workgroup that waits for another, so the list does not depend on the launch grid or on scheduling:
//
//   count  item = a chunk of 256 consecutive k (4 waves x 64 lanes, one node per lane).  A lane reads the TURB
//          taps of its node alone; the wave's 64-bit ballot of the predicate goes to masks[k / 64] and the
//          chunk's popcount to counts[item] (the four waves meet in LDS, one barrier per item).
//   scan   one workgroup turns counts[0 .. items) into exclusive offsets in place (integers: exact in any
//          order) and writes the header record (T, W = min(T, capacity), nx * ny, capacity, 0, 0, 0, 0).
//   emit   item = the same chunk.  rank = the chunk's offset + the popcounts of the chunk's earlier waves + the
//          popcount of the wave's mask below the lane.  Only selected lanes with rank < capacity sample DISP,
//          VEL and the foam and store their two float4; a chunk without a selected node is skipped, and at the
//          first chunk whose offset reaches the capacity the workgroup is done (offsets only grow).
//
// count and emit walk their items with launch_items under OCEAN_MAX_GROUPS, like the frame kernels.  A gather
// through L1 / L2 / Infinity Cache like the grid kernel's: no roofline claimed.  No inline assembly.
#include "ocean_internal.h"
#include "sample_filter.h"

namespace ocean {
namespace {

constexpr int kThreads = 256, kWaves = kThreads / 64;  // a chunk = one node per lane

// Node k of the grid: (qx, qz), one fp32 multiply and one fp32 add each (ocean.h).
__device__ __forceinline__ float2 node_at(unsigned k, unsigned nx, float x0, float z0, float dx, float dz) {
    const unsigned j = k / nx, i = k - j * nx;
    return make_float2(x0 + (float)i * dx, z0 + (float)j * dz);
}

__global__ __launch_bounds__(kThreads) void k_whitecap_count(DevView v, int tile, float lod, float threshold, float x0,
                                                             float z0, float dx, float dz, unsigned nx, unsigned nodes,
                                                             unsigned items, unsigned long long* __restrict__ masks,
                                                             unsigned* __restrict__ counts) {
    // the waves' popcounts, in two buffers taken in turn: thread 0 has read an item's buffer before it reaches the
    // next item's barrier, and the waves write that buffer again only behind that barrier: one barrier per item
    __shared__ unsigned part[2][kWaves];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned turn = 0;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x, turn ^= 1u) {
        const unsigned k = item * kThreads + threadIdx.x;
        bool sel = false;
        if (k < nodes) {
            const float2 q = node_at(k, nx, x0, z0, dx, dz);
            sel = sample_foam(v, tile, q.x, q.y, lod) >= threshold;  // false for a NaN foam
        }
        const unsigned long long m = __ballot(sel);
        if (lane == 0) {
            masks[(size_t)item * kWaves + wave] = m;  // word k / 64; zero past the last node
            part[turn][wave] = (unsigned)__popcll(m);
        }
        __syncthreads();
        if (threadIdx.x == 0) counts[item] = (part[turn][0] + part[turn][1]) + (part[turn][2] + part[turn][3]);
    }
}

// One workgroup.  Lane t owns the items [t * per, (t + 1) * per): it sums them, the workgroup scans the 256
// sums, and the lane writes its items' exclusive offsets from its own.  The header's third field is `nodes`, or
// *nodes_dev where the candidates are counted on the device (the spray particles, spray.hip).
__global__ __launch_bounds__(kThreads) void k_whitecap_scan(unsigned* __restrict__ counts, unsigned items,
                                                            unsigned nodes, const unsigned* __restrict__ nodes_dev,
                                                            unsigned capacity, uint4* __restrict__ header) {
    __shared__ unsigned wsum[kWaves];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned per = (items + kThreads - 1) / kThreads;
    const unsigned lo = min(threadIdx.x * per, items), hi = min(lo + per, items);
    unsigned sum = 0;
    for (unsigned i = lo; i < hi; ++i) sum += counts[i];
    unsigned incl = sum;
    for (int s = 1; s < 64; s <<= 1) {
        const unsigned t = __shfl_up(incl, s, 64);
        if ((int)lane >= s) incl += t;
    }
    if (lane == 63) wsum[wave] = incl;
    __syncthreads();
    unsigned before = 0, total = 0;
    for (unsigned w = 0; w < (unsigned)kWaves; ++w) {
        if (w < wave) before += wsum[w];
        total += wsum[w];
    }
    unsigned run = before + incl - sum;
    for (unsigned i = lo; i < hi; ++i) {
        const unsigned c = counts[i];
        counts[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) {
        header[0] = make_uint4(total, min(total, capacity), nodes_dev ? *nodes_dev : nodes, capacity);
        header[1] = make_uint4(0u, 0u, 0u, 0u);
    }
}

__global__ __launch_bounds__(kThreads) void k_whitecap_emit(DevView v, const float4* __restrict__ vel, int tile,
                                                            float lod, float x0, float z0, float dx, float dz,
                                                            unsigned nx, unsigned items, unsigned capacity,
                                                            const unsigned long long* __restrict__ masks,
                                                            const unsigned* __restrict__ offsets,
                                                            float4* __restrict__ records) {
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    for (unsigned item = blockIdx.x; item < items; item += gridDim.x) {
        unsigned rank = offsets[item];
        if (rank >= capacity) break;  // so is every later chunk's
        const unsigned long long* cm = masks + (size_t)item * kWaves;
        for (unsigned w = 0; w < wave; ++w) rank += (unsigned)__popcll(cm[w]);
        const unsigned long long m = cm[wave];
        if (m == 0 || rank >= capacity) continue;  // wave-uniform
        rank += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
        if (!((m >> lane) & 1ull) || rank >= capacity) continue;
        const unsigned k = item * kThreads + threadIdx.x;
        const float2 q = node_at(k, nx, x0, z0, dx, dz);
        const float4 d = sample_disp(v, tile, q.x, q.y);
        float4 vs = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (vel) vs = sample_velocity(v, vel, tile, q.x, q.y);  // ocean_query_velocity's Vs(q) with no fixed-point step
        float4* o = records + 2 * (size_t)rank;
        o[0] = make_float4(q.x + d.x, d.y, q.y + d.z, sample_foam(v, tile, q.x, q.y, lod));
        o[1] = make_float4(vs.x, vs.y, vs.z, (float)k);  // k < 2^22: exact
    }
}

}  // namespace

hipError_t launch_compact_scan(unsigned* counts, unsigned items, unsigned nodes, const unsigned* nodes_dev,
                               unsigned capacity, float* out, hipStream_t s) {
    launch(k_whitecap_scan, dim3(1), dim3(kThreads), 0, s, counts, items, nodes, nodes_dev, capacity,
           reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

size_t whitecap_scratch_bytes() {
    return (size_t)(OCEAN_GRID_MAX_NODES / 64) * sizeof(unsigned long long) +
           (size_t)(OCEAN_GRID_MAX_NODES / kThreads) * sizeof(unsigned);
}

hipError_t launch_whitecaps(const DevView& v, const float4* vel, int tile, float lod, float threshold, float x0, float z0,
                            float dx, float dz, int nx, int ny, int capacity, void* scratch, float* out, hipStream_t s) {
    if (nx <= 0 || ny <= 0 || capacity <= 0 || (uint64_t)nx * (uint64_t)ny > (uint64_t)OCEAN_GRID_MAX_NODES)
        return hipErrorInvalidValue;
    const unsigned nodes = (unsigned)nx * (unsigned)ny;
    const unsigned items = (nodes + kThreads - 1) / kThreads;  // <= 2^22 / 256: the scratch holds every grid
    unsigned long long* masks = static_cast<unsigned long long*>(scratch);
    unsigned* counts = reinterpret_cast<unsigned*>(masks + OCEAN_GRID_MAX_NODES / 64);
    const Items it{(int)items, v.max_groups};
    hipError_t e = launch_items(k_whitecap_count, kThreads, it, s, v, tile, lod, threshold, x0, z0, dx, dz, (unsigned)nx,
                                nodes, items, masks, counts);
    if (e != hipSuccess) return e;
    e = launch_compact_scan(counts, items, nodes, nullptr, (unsigned)capacity, out, s);
    if (e != hipSuccess) return e;
    return launch_items(k_whitecap_emit, kThreads, it, s, v, vel, tile, lod, x0, z0, dx, dz, (unsigned)nx, items,
                        (unsigned)capacity, (const unsigned long long*)masks, (const unsigned*)counts,
                        reinterpret_cast<float4*>(out) + 2);
}

}  // namespace ocean
