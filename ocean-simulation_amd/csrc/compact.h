// Order-preserving stream compaction, shared by the whitecap emitters (whitecaps.hip) and the spray particles
// (spray.hip): candidates k = 0, 1, ... each carry a predicate, and candidate k with a true predicate writes
// record 1 + rank(k), rank(k) = the selected candidates below k, while rank(k) < capacity.  Three launches, with
// no atomics and no workgroup that waits for another, so the list does not depend on the launch grid or on
// scheduling:
//
//   count  the consumer's kernel.  item = a chunk of 256 consecutive candidates (4 waves x 64 lanes, one candidate
//          per lane).  A lane evaluates its own predicate and hands it to compact_count: the wave's 64-bit ballot
//          goes to masks[k / 64] and the chunk's popcount to counts[item].
//   scan   k_whitecap_scan (compact.hip), one workgroup: counts[0 .. items) become exclusive offsets in place
//          (integers: exact in any order), and the header record (T, W = min(T, capacity), candidates, capacity,
//          0, 0, 0, 0) is written.
//   emit   the consumer's kernel over the same chunks.  compact_rank gives a selected lane its rank, and the lane
//          writes its two float4 to records + 2 * rank.
//
// Both consumer kernels walk their items with launch_items under OCEAN_MAX_GROUPS, like the frame kernels.  The
// statements of the two device functions are in the order the kernels had them before they were shared: that
// order decides the machine code (docs/MEASUREMENTS.md section 29).  No inline assembly.
//
// The launches meet in a scratch block whose layout compact_scratch states once, for the host.
#pragma once

#include "ocean_internal.h"

namespace ocean {

constexpr int kChunkThreads = 256, kChunkWaves = kChunkThreads / 64;  // a chunk = one candidate per lane

// The end of a count kernel's item: publishes this lane's predicate `sel` for chunk `item`.  Every lane of the
// workgroup calls it once per item (it holds a barrier), with `turn` = 0 before the first item.
// The waves' popcounts meet in LDS, in two buffers taken in turn: thread 0 has read an item's buffer before it
// reaches the next item's barrier, and the waves write that buffer again only behind that barrier.  So one
// barrier per item suffices.
__device__ __forceinline__ void compact_count(bool sel, unsigned item, unsigned& turn,
                                              unsigned long long* __restrict__ masks, unsigned* __restrict__ counts) {
    __shared__ unsigned part[2][kChunkWaves];
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const unsigned long long m = __ballot(sel);
    if (lane == 0) {
        masks[(size_t)item * kChunkWaves + wave] = m;  // word k / 64; zero past the last candidate
        part[turn][wave] = (unsigned)__popcll(m);
    }
    __syncthreads();
    if (threadIdx.x == 0) counts[item] = (part[turn][0] + part[turn][1]) + (part[turn][2] + part[turn][3]);
    turn ^= 1u;
}

// What an emit kernel asks per item for this lane's candidate in chunk `item`: true, and its rank below the
// capacity in `rank`, when the lane has a record to write; else false, with `done` saying whether the workgroup
// is done: the chunk's offset has reached the capacity, and so has every later chunk's (offsets only grow).
// rank = the chunk's offset + the popcounts of the chunk's earlier waves + the popcount of the wave's mask below
// the lane.  A wave without a selected candidate, or whose first rank has reached the capacity, leaves before the
// per-lane arithmetic (wave-uniform); then a lane that is not selected or whose own rank has reached it.
__device__ __forceinline__ bool compact_rank(unsigned item, const unsigned* __restrict__ offsets,
                                             const unsigned long long* __restrict__ masks, unsigned capacity,
                                             unsigned& rank, bool& done) {
    const unsigned wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    rank = offsets[item];
    done = rank >= capacity;
    if (done) return false;
    const unsigned long long* cm = masks + (size_t)item * kChunkWaves;
    for (unsigned w = 0; w < wave; ++w) rank += (unsigned)__popcll(cm[w]);
    const unsigned long long m = cm[wave];
    if (m == 0 || rank >= capacity) return false;  // wave-uniform
    rank += (unsigned)__popcll(m & ((1ull << lane) - 1ull));
    return ((m >> lane) & 1ull) && rank < capacity;
}

// Where the three launches of a compaction over `items` chunks meet, as byte offsets into a 16-B aligned block:
// an optional payload of `payload` bytes per candidate (a multiple of 16) that the count kernel leaves for the
// emit kernel, the ballot masks (8-B words, four per chunk), the per-chunk counts (padded to a multiple of 16 B)
// and, where the candidates are counted on the device (`total`), that count in 16 B of its own.
struct CompactScratch {
    size_t payload, masks, counts, total, bytes;
};
inline CompactScratch compact_scratch(size_t items, size_t payload, bool total) {
    CompactScratch at;
    at.payload = 0;
    at.masks = items * kChunkThreads * payload;
    at.counts = at.masks + items * kChunkWaves * sizeof(unsigned long long);
    at.total = at.counts + ((items + 3) & ~(size_t)3) * sizeof(unsigned);
    at.bytes = at.total + (total ? 16 : 0);
    return at;
}
template <class T>
inline T* scratch_at(void* block, size_t offset) {
    return reinterpret_cast<T*>(static_cast<char*>(block) + offset);
}

}  // namespace ocean
