// Item table of the pruned pass AQ (fftq.hip, DESIGN.md section 3 "Band-limited cascades"): host code,
// no HIP (tests/prune_items_test.cpp builds it alone).
//
// Unit u of a context has the live extent m_u: the largest |y - N/2| over the rows y of its h0k that hold
// a non-zero texel, -1 when it holds none, N/2 when row 0 is live (dense).  Item i of a unit is rows i and
// (N - i) % N, both N/2 - i from the centre row, so the live items of unit u are i = N/2 - m_u .. N/2.
// The table lists them unit by unit, i ascending, one packed int each; the items of a chunk of units
// [u0, u0 + nu) are the contiguous range [pre[u0], pre[u0 + nu]).
#pragma once

#include <vector>

namespace ocean {

constexpr int kPruneRowBits = 16;             // item = u << 16 | y1
constexpr int kPruneMaxUnits = 1 << 15;       // u << 16 stays a non-negative int
constexpr int prune_pack(int u, int y1) { return (u << kPruneRowBits) | y1; }
constexpr int prune_unit(int item) { return item >> kPruneRowBits; }
constexpr int prune_row(int item) { return item & ((1 << kPruneRowBits) - 1); }

struct PruneItems {
    std::vector<int> pre;    // [units + 1]: items before unit u
    std::vector<int> items;  // [pre[units]]: prune_pack(u, y1)
    bool dense = true;       // every extent is N/2: nothing to skip

    // ext[u] = m_u in [-1, n / 2]; values outside are clamped (a corrupt readback cannot index out of a row)
    void build(const int* ext, int units, int n) {
        pre.assign((size_t)units + 1, 0);
        items.clear();
        dense = true;
        for (int u = 0; u < units; ++u) {
            const int m = ext[u] < -1 ? -1 : (ext[u] > n / 2 ? n / 2 : ext[u]);
            dense = dense && m == n / 2;
            for (int i = n / 2 - m; i <= n / 2; ++i) items.push_back(prune_pack(u, i));
            pre[(size_t)u + 1] = (int)items.size();
        }
    }
    // first item and item count of the units [u0, u0 + nu)
    void chunk(int u0, int nu, int* first, int* count) const {
        *first = pre[(size_t)u0];
        *count = pre[(size_t)u0 + nu] - pre[(size_t)u0];
    }
};

}  // namespace ocean
