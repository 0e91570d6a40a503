// Stand-alone check of pass AQ's item table (ocean-simulation_amd/csrc/prune_items.h) against brute force:
// random live extents m_u in [-1, N/2] for up to 8 units at N = 512; the count, the (u, y1) of every item in
// order, every chunk's sub-range and the empty chunk.  tests/test_prune_items.py builds and runs it.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "prune_items.h"

namespace {

int failures = 0;
#define CHECK(cond, ...)                 \
    do {                                 \
        if (!(cond)) {                   \
            std::printf("FAIL: ");       \
            std::printf(__VA_ARGS__);    \
            std::printf("\n");           \
            if (++failures > 20) std::exit(1); \
        }                                \
    } while (0)

unsigned long long rng_state = 0x9E3779B97F4A7C15ull;
unsigned rnd() {
    rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
    return (unsigned)(rng_state >> 33);
}

// brute force: every (u, i) in the dense order, kept when row i is within m_u of the centre row
std::vector<int> brute(const std::vector<int>& ext, int u0, int nu, int n) {
    std::vector<int> out;
    for (int u = u0; u < u0 + nu; ++u)
        for (int i = 0; i <= n / 2; ++i) {
            const int y1 = i, y2 = (n - i) % n;
            const int d1 = std::abs(y1 - n / 2), d2 = std::abs(y2 - n / 2);
            if (d1 != d2) {
                std::printf("FAIL: rows %d and %d of item %d are not equally far from the centre\n", y1, y2, i);
                std::exit(1);
            }
            if (d1 <= ext[(size_t)u]) out.push_back(ocean::prune_pack(u, y1));
        }
    return out;
}

void check_case(const std::vector<int>& ext, int n) {
    const int U = (int)ext.size();
    ocean::PruneItems t;
    t.build(ext.data(), U, n);
    const std::vector<int> want = brute(ext, 0, U, n);
    CHECK(t.items.size() == want.size(), "count %zu != %zu", t.items.size(), want.size());
    CHECK((int)t.pre.size() == U + 1 && t.pre[0] == 0 && t.pre[(size_t)U] == (int)t.items.size(), "prefix ends");
    bool dense = true;
    for (int u = 0; u < U; ++u) dense = dense && ext[(size_t)u] == n / 2;
    CHECK(t.dense == dense, "dense flag %d != %d", (int)t.dense, (int)dense);
    for (size_t k = 0; k < want.size() && k < t.items.size(); ++k) {
        CHECK(t.items[k] == want[k], "item %zu: (%d, %d) != (%d, %d)", k, ocean::prune_unit(t.items[k]),
              ocean::prune_row(t.items[k]), ocean::prune_unit(want[k]), ocean::prune_row(want[k]));
        CHECK(ocean::prune_row(t.items[k]) <= n / 2 && ocean::prune_unit(t.items[k]) < U, "item %zu out of range", k);
    }
    // every chunk [u0, u0 + nu), the empty ones included
    for (int u0 = 0; u0 <= U; ++u0)
        for (int nu = 0; u0 + nu <= U; ++nu) {
            int first = -1, count = -1;
            t.chunk(u0, nu, &first, &count);
            const std::vector<int> w = brute(ext, u0, nu, n);
            CHECK(count == (int)w.size(), "chunk (%d, %d): count %d != %zu", u0, nu, count, w.size());
            CHECK(first >= 0 && first + count <= (int)t.items.size(), "chunk (%d, %d) outside the table", u0, nu);
            for (int k = 0; k < count && k < (int)w.size(); ++k)
                CHECK(t.items[(size_t)first + k] == w[(size_t)k], "chunk (%d, %d) item %d", u0, nu, k);
        }
}

}  // namespace

int main() {
    const int n = 512;
    check_case({}, n);                        // no unit
    check_case({-1}, n);                      // a flat unit: no item
    check_case({-1, -1, -1}, n);              // the empty chunk of several units
    check_case({0}, n);                       // the centre row alone
    check_case({n / 2}, n);                   // dense
    check_case({n / 2 - 1}, n);               // all rows but row 0
    check_case({n / 2, 54, -1, n / 2}, n);    // mixed, as a cascaded ocean
    for (int rep = 0; rep < 200; ++rep) {
        std::vector<int> ext(1 + rnd() % 8);
        for (int& m : ext) {
            const unsigned k = rnd() % 8;
            m = k == 0 ? -1 : (k == 1 ? n / 2 : (int)(rnd() % (unsigned)(n / 2 + 2)) - 1);
        }
        check_case(ext, n);
    }
    // a corrupt extent cannot index outside a row
    {
        const int bad[2] = {-7, n};
        ocean::PruneItems t;
        t.build(bad, 2, n);
        CHECK(t.pre[1] == 0 && t.pre[2] == n / 2 + 1, "clamped extents");
    }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
