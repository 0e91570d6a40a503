// The scan between a compaction's count and emit launches (compact.h).  Its kernel keeps the name it had when the
// whitecap emitters were the only consumer, so profiles and ocean_kernel_name read the same symbol.
#include "compact.h"

namespace ocean {
namespace {

// One workgroup.  Lane t owns the items [t * per, (t + 1) * per): it sums them, the workgroup scans the 256
// sums, and the lane writes its items' exclusive offsets from its own.  The header's third field is `nodes`, or
// *nodes_dev where the candidates are counted on the device (the spray particles, spray.hip).
__global__ __launch_bounds__(kChunkThreads) void k_whitecap_scan(unsigned* __restrict__ counts, unsigned items,
                                                                 unsigned nodes, const unsigned* __restrict__ nodes_dev,
                                                                 unsigned capacity, uint4* __restrict__ header) {
    __shared__ unsigned wsum[kChunkWaves];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned per = (items + kChunkThreads - 1) / kChunkThreads;
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
    for (unsigned w = 0; w < (unsigned)kChunkWaves; ++w) {
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

}  // namespace

hipError_t launch_compact_scan(unsigned* counts, unsigned items, unsigned nodes, const unsigned* nodes_dev,
                               unsigned capacity, float* out, hipStream_t s) {
    launch(k_whitecap_scan, dim3(1), dim3(kChunkThreads), 0, s, counts, items, nodes, nodes_dev, capacity,
           reinterpret_cast<uint4*>(out));
    return hipGetLastError();
}

}  // namespace ocean
