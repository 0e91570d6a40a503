// Stand-alone check of the frame schedule (ocean-simulation_amd/csrc/frame_plan.h): the steps plan_frame hands
// out, in order, for the benchmark shapes and for every choice the schedule makes, against plans derived by hand
// at each case.  tests/test_frame_plan.py builds and runs it; any argument prints every plan.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "frame_plan.h"

namespace {

using ocean::FrameInputs;
using ocean::FramePass;
using ocean::FrameStep;
using Plan = std::vector<FrameStep>;

int failures = 0;
bool verbose = false;
#define CHECK(cond, ...)                       \
    do {                                       \
        if (!(cond)) {                         \
            std::printf("FAIL line %d: ", __LINE__); \
            std::printf(__VA_ARGS__);          \
            std::printf("\n");                 \
            if (++failures > 40) std::exit(1); \
        }                                      \
    } while (0)

const char* pass_name(FramePass p) {
    static const char* const names[] = {"A_Q", "A_V4", "A_V3", "B_Q", "B_V3", "C4", "C4Q"};
    return names[(int)p];
}

// A context as ocean_create and ocean_init_spectrum leave it: default knobs, h0k and the side arrays where the
// size has them, the spectrum generated (h0k valid, h0.zw conjugate), dense extents.  `prune` must outlive the
// inputs.  finish() sizes the intermediate and builds the item table, after a case has changed shape or knobs.
struct Ctx {
    FrameInputs in{};
    ocean::PruneItems prune;
    Ctx(int n, int C, int T, int P = 4) {
        in.shape = {n, C, T, P, 0, 0, n, -1};
        in.knobs = {1, 1, 192, 0, -1};
        finish(std::vector<int>((size_t)T * C, n / 2));
    }
    void finish(const std::vector<int>& ext) {
        const ocean::FrameShape& sh = in.shape;
        in.state = {ocean::pass_a4_supported(sh.n, sh.P), ocean::pass_q_supported(sh.n, sh.P), false, true, false, &prune};
        in.state.h0k_valid = in.state.h0k;
        in.shape.inter_units = ocean::inter_units(in);
        prune.build(ext.data(), (int)ext.size(), sh.n);
        in.state.prune_ready = ocean::prune_tables(in);
    }
    void finish() { finish(std::vector<int>((size_t)in.units(), in.shape.n / 2)); }
};

Plan plan(const Ctx& c, const char* what) {
    Plan p;
    const int r = ocean::plan_frame(c.in, [&](const FrameStep& st) {
        p.push_back(st);
        return 0;
    });
    CHECK(r == 0, "%s: plan_frame returned %d", what, r);
    if (verbose) {
        std::printf("%s: N %d C %d T %d P %d, intermediate of %zu units\n", what, c.in.shape.n, c.in.shape.C, c.in.shape.T,
                    c.in.shape.P, c.in.shape.inter_units);
        for (const FrameStep& s : p) {
            std::printf("  %-4s kind %d %s units [%d, +%d) slot %d%s x [%d, +%d)%s", pass_name(s.pass), s.kind, s.name, s.u0,
                        s.nu, s.inter_u0, s.inter_at_base ? " at base" : "", s.x0, s.nx, s.disp_cached ? " disp cached" : "");
            if (s.pruned) std::printf(" pruned: items [%d, +%d) ubase %d", s.first, s.items, s.ubase);
            std::printf("\n");
        }
    }
    return p;
}

// step k of the plan is `pass` over units [u0, u0 + nu)
void expect(const Plan& p, size_t k, FramePass pass, int u0, int nu, const char* what) {
    if (k >= p.size()) {
        CHECK(false, "%s: no step %zu (the plan has %zu)", what, k, p.size());
        return;
    }
    const FrameStep& s = p[k];
    CHECK(s.pass == pass && s.u0 == u0 && s.nu == nu, "%s: step %zu is %s(%d, %d), not %s(%d, %d)", what, k, pass_name(s.pass),
          s.u0, s.nu, pass_name(pass), u0, nu);
    const bool row_pass = pass == FramePass::A_Q || pass == FramePass::A_V4 || pass == FramePass::A_V3;
    CHECK(s.kind == (row_pass ? 0 : 1), "%s: step %zu has kind %d", what, k, s.kind);
}

void count_kinds(const Plan& p, int* k0, int* k1) {
    *k0 = *k1 = 0;
    for (const FrameStep& s : p) ++*(s.kind == 0 ? k0 : k1);
}

void benchmark_shapes() {
    {
        // cfg3: a three-plane unit is 1024^2 x 8 B x 3 = 24 MiB, 192 / 24 = 8 units, whole tiles: 8, at least U = 4:
        // K = 4, one chunk.  Re-read set plus DISP: 4 x 2^20 x (8 + 24 + 4 + 16) B = 208 MiB <= 224 MiB: DISP cached.
        // Dense extents: unpruned.
        Ctx c(1024, 4, 1);
        const Plan p = plan(c, "cfg3");
        CHECK(c.in.shape.inter_units == 4 && p.size() == 2, "cfg3: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        expect(p, 0, FramePass::A_Q, 0, 4, "cfg3");
        expect(p, 1, FramePass::B_Q, 0, 4, "cfg3");
        for (const FrameStep& s : p)
            CHECK(!s.pruned && s.disp_cached && !s.inter_at_base && s.x0 == 0 && s.nx == 1024, "cfg3 %s", pass_name(s.pass));
        CHECK(p.size() == 2 && p[0].name[5] == 'a' && p[1].name[5] == 'b', "cfg3 names");
    }
    {
        // cfg3's scene: cascades 0..2 dense (513 items each), cascade 3 with extent 54 (55 items):
        // 3 x 513 + 55 = 1594 of 2052; 1594 x 8 = 12752 <= 2052 x 7 = 14364: both passes pruned.
        Ctx c(1024, 4, 1);
        c.finish({512, 512, 512, 54});
        const Plan p = plan(c, "cfg3 band-limited");
        expect(p, 0, FramePass::A_Q, 0, 4, "cfg3 band-limited");
        expect(p, 1, FramePass::B_Q, 0, 4, "cfg3 band-limited");
        for (const FrameStep& s : p)
            CHECK(s.pruned && s.first == 0 && s.items == 1594 && s.ubase == 0 && s.disp_cached, "cfg3 band-limited: items %d",
                  s.items);
    }
    {
        // every extent -1: 0 live items, 0 <= 2052 x 7: pruned; a chunk with no live item launches no pass A
        Ctx c(1024, 4, 1);
        c.finish({-1, -1, -1, -1});
        const Plan p = plan(c, "flat sea");
        CHECK(p.size() == 1, "flat sea: %zu steps", p.size());
        expect(p, 0, FramePass::B_Q, 0, 4, "flat sea");
        CHECK(!p.empty() && p[0].pruned && p[0].items == 0, "flat sea: pass B is pruned with no item");
    }
    {
        // cfg4: a three-plane unit is 512^2 x 8 x 3 = 6 MiB, 192 / 6 = 32 units, a multiple of C = 4; a four-plane one
        // 8 MiB, 24 units: the intermediate holds 32, K = 32, 1024 / 32 = 32 chunks that all reuse it from the base.
        // More than one chunk: DISP is not cached.
        Ctx c(512, 4, 256);
        const Plan p = plan(c, "cfg4");
        CHECK(c.in.shape.inter_units == 32 && p.size() == 64, "cfg4: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        for (size_t k = 0; k < p.size(); ++k) {
            expect(p, k, k % 2 ? FramePass::B_Q : FramePass::A_Q, 32 * (int)(k / 2), 32, "cfg4");
            CHECK(p[k].inter_at_base && p[k].inter_u0 == 0 && !p[k].disp_cached && !p[k].pruned, "cfg4 step %zu", k);
        }
    }
    {
        // cfg5: a unit of the three-plane frame at N >= 2048 has four planes, 4096^2 x 8 x 4 = 512 MiB > 192: larger
        // than a chunk, so the whole frame is one chunk, K = 4.  One band's planes: 512 MiB > 256 MiB, two bands of
        // 2048 columns (a multiple of 16).  Pass A once, then the column passes per (unit, band), each unit in its own slot.
        Ctx c(4096, 4, 1);
        const Plan p = plan(c, "cfg5");
        CHECK(c.in.shape.inter_units == 4 && p.size() == 9, "cfg5: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        expect(p, 0, FramePass::A_Q, 0, 4, "cfg5");
        for (size_t k = 1; k < p.size(); ++k) {
            const int u = (int)(k - 1) / 2, b = (int)(k - 1) % 2;
            expect(p, k, FramePass::C4Q, u, 1, "cfg5");
            CHECK(p[k].x0 == 2048 * b && p[k].nx == 2048 && p[k].inter_u0 == u && !p[k].inter_at_base, "cfg5 step %zu", k);
            CHECK(!p[k].disp_cached && !p[k].pruned && p[k].name[5] == 'c', "cfg5 step %zu", k);
        }
    }
    {
        // cfg2: displacement only, no three-plane frame; N = 512 with two planes has the mirror-pair row pass
        Ctx c(512, 1, 1, 2);
        const Plan p = plan(c, "cfg2");
        CHECK(p.size() == 2, "cfg2: %zu steps", p.size());
        expect(p, 0, FramePass::A_V4, 0, 1, "cfg2");
        expect(p, 1, FramePass::B_V3, 0, 1, "cfg2");
    }
}

void frame_kinds() {
    {
        // N = 2048 keeps the four-plane passes and has no mirror-pair row pass.  A unit is 2048^2 x 8 x 4 = 128 MiB:
        // K = 1 = U; one band's planes are 128 MiB <= 256 MiB: one band, one launch for the chunk ("pass_b").
        Ctx c(2048, 1, 1);
        const Plan p = plan(c, "2048");
        CHECK(p.size() == 2, "2048: %zu steps", p.size());
        expect(p, 0, FramePass::A_V3, 0, 1, "2048");
        expect(p, 1, FramePass::C4, 0, 1, "2048");
        CHECK(p.size() == 2 && p[1].x0 == 0 && p[1].nx == 2048 && p[1].name[5] == 'b', "2048: the column step");
    }
    {
        // after an H0 upload h0k is stale and h0.zw arbitrary: the four-plane frame with per-texel rows, never pruned
        Ctx c(1024, 4, 1);
        c.finish({512, 512, 512, 54});
        c.in.state.h0k_valid = c.in.state.h0_conj = false;
        const Plan p = plan(c, "1024 after an H0 upload");
        CHECK(p.size() == 2, "upload: %zu steps", p.size());
        expect(p, 0, FramePass::A_V3, 0, 4, "upload");
        expect(p, 1, FramePass::B_V3, 0, 4, "upload");
        for (const FrameStep& s : p) CHECK(!s.pruned && !s.disp_cached, "upload: %s", pass_name(s.pass));
    }
    {
        // OCEAN_A4=0 with a valid spectrum: at N <= 1024 the three-plane frame needs the mirror-pair row pass, so
        // the four-plane frame runs, with per-texel rows
        Ctx c(1024, 4, 1);
        c.in.knobs.a4 = 0;
        const Plan p = plan(c, "1024, OCEAN_A4=0");
        expect(p, 0, FramePass::A_V3, 0, 4, "a4 = 0");
        expect(p, 1, FramePass::B_V3, 0, 4, "a4 = 0");
        c.in.knobs = {0, 1, 192, 0, -1};  // OCEAN_Q=0 alone: four planes, mirror-pair rows
        const Plan q0 = plan(c, "1024, OCEAN_Q=0");
        expect(q0, 0, FramePass::A_V4, 0, 4, "q = 0");
        expect(q0, 1, FramePass::B_V3, 0, 4, "q = 0");
    }
}

void dead_share() {
    // N = 512, 8 units in one chunk (6 MiB each): 8 x 257 = 2056 items.  Seven dense units and a flat one: 1799 live,
    // exactly an eighth dead, 1799 x 8 = 14392 <= 2056 x 7 = 14392: pruned.  The eighth unit with its centre row
    // live: 1800 x 8 = 14400 > 14392: the dense kernels, though the table is not dense.
    for (int last : {-1, 0}) {
        Ctx c(512, 4, 2);
        c.finish({256, 256, 256, 256, 256, 256, 256, last});
        const Plan p = plan(c, last < 0 ? "an eighth dead" : "just under an eighth dead");
        CHECK(p.size() == 2 && !c.prune.dense, "dead share: %zu steps", p.size());
        for (const FrameStep& s : p) CHECK(s.pruned == (last < 0), "dead share %d: %s pruned %d", last, pass_name(s.pass), s.pruned);
        if (last < 0 && p.size() == 2) CHECK(p[0].items == 1799 && p[1].items == 1799, "dead share: items %d", p[0].items);
    }
    CHECK(ocean::prune_pays(7, 8) && !ocean::prune_pays(8, 8) && ocean::prune_pays(0, 1), "prune_pays");
}

void chunks() {
    {
        // OCEAN_CHUNK_MIB=0: the whole frame at once
        Ctx c(512, 4, 16);
        c.in.knobs.chunk_mib = 0;
        c.finish();
        const Plan p = plan(c, "chunk_mib 0");
        CHECK(c.in.shape.inter_units == 64 && p.size() == 2, "chunk_mib 0: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        expect(p, 0, FramePass::A_Q, 0, 64, "chunk_mib 0");
        expect(p, 1, FramePass::B_Q, 0, 64, "chunk_mib 0");
        CHECK(p.size() == 2 && !p[0].inter_at_base, "chunk_mib 0");
    }
    {
        // a unit larger than a chunk (24 MiB against 16): the whole frame is one chunk
        Ctx c(1024, 4, 2);
        c.in.knobs.chunk_mib = 16;
        c.finish();
        const Plan p = plan(c, "unit larger than a chunk");
        CHECK(c.in.shape.inter_units == 8 && p.size() == 2, "large unit: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        expect(p, 0, FramePass::A_Q, 0, 8, "large unit");
    }
    {
        // N = 512, C = 3, T = 2, 12 MiB: two three-plane units (6 MiB) per chunk, fewer than a tile, so chunks start
        // mid-tile: units (0, 1), (2, 3), (4, 5); one four-plane unit (8 MiB): the intermediate holds 2 units, reused.
        // With extents (dense, flat, sparse) per tile the chunks hold 257 + 0, 55 + 257 and 0 + 55 live items of 514.
        Ctx c(512, 3, 2);
        c.in.knobs.chunk_mib = 12;
        c.finish({256, -1, 54, 256, -1, 54});
        const Plan p = plan(c, "chunks that start mid-tile");
        CHECK(c.in.shape.inter_units == 2 && p.size() == 6, "mid-tile: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        const int first[3] = {0, 257, 569}, items[3] = {257, 312, 55};
        for (size_t k = 0; k < p.size(); ++k) {
            const int ch = (int)k / 2;
            expect(p, k, k % 2 ? FramePass::B_Q : FramePass::A_Q, 2 * ch, 2, "mid-tile");
            CHECK(p[k].inter_at_base && p[k].inter_u0 == 0 && !p[k].disp_cached, "mid-tile step %zu", k);
            CHECK(p[k].pruned && p[k].first == first[ch] && p[k].items == items[ch] && p[k].ubase == 2 * ch,
                  "mid-tile step %zu: items [%d, +%d) ubase %d", k, p[k].first, p[k].items, p[k].ubase);
        }
        // the same shape dense: three row and three column launches; flat: no row launch
        int k0, k1;
        c.finish();
        count_kinds(plan(c, "mid-tile, dense"), &k0, &k1);
        CHECK(k0 == 3 && k1 == 3, "mid-tile dense: %d + %d launches", k0, k1);
        c.finish({-1, -1, -1, -1, -1, -1});
        count_kinds(plan(c, "mid-tile, flat"), &k0, &k1);
        CHECK(k0 == 0 && k1 == 3, "mid-tile flat: %d + %d launches", k0, k1);
    }
    {
        // chunks and bands together.  N = 2048, displacement only, 4 tiles, OCEAN_C4_BANDS=2: a unit is 2048^2 x 8 x 2
        // = 64 MiB, K = 3, the intermediate holds 3 units and every chunk starts at its base.  Chunk (0, 1, 2): one row
        // launch, then unit u of the chunk in slot u, two bands each; chunk (3): unit 3 in slot 0.
        Ctx c(2048, 1, 4, 2);
        c.in.knobs.c4_bands = 2;
        c.finish();
        const Plan p = plan(c, "chunks of banded units");
        CHECK(c.in.shape.inter_units == 3 && p.size() == 10, "banded chunks: %zu units, %zu steps", c.in.shape.inter_units, p.size());
        expect(p, 0, FramePass::A_V3, 0, 3, "banded chunks");
        expect(p, 7, FramePass::A_V3, 3, 1, "banded chunks");
        const int unit[10] = {0, 0, 0, 1, 1, 2, 2, 3, 3, 3}, slot[10] = {0, 0, 0, 1, 1, 2, 2, 0, 0, 0};
        for (size_t k = 0; k < p.size(); ++k) {
            CHECK(p[k].inter_at_base && p[k].inter_u0 == slot[k], "banded chunks step %zu: slot %d", k, p[k].inter_u0);
            if (k == 0 || k == 7) continue;
            expect(p, k, FramePass::C4, unit[k], 1, "banded chunks");
            const int b = (int)(k > 7 ? k - 8 : k - 1) % 2;
            CHECK(p[k].x0 == 1024 * b && p[k].nx == 1024 && p[k].name[5] == 'c', "banded chunks step %zu: x [%d, +%d)", k,
                  p[k].x0, p[k].nx);
        }
    }
}

void column_bands() {
    {
        // a column band context is never pruned, and every step carries the band
        Ctx c(1024, 4, 1);
        c.in.shape.band_x0 = 256;
        c.in.shape.band_nx = 512;
        c.finish({512, 512, 512, 54});
        const Plan p = plan(c, "column band");
        expect(p, 0, FramePass::A_Q, 0, 4, "column band");
        expect(p, 1, FramePass::B_Q, 0, 4, "column band");
        for (const FrameStep& s : p) CHECK(!s.pruned && s.x0 == 256 && s.nx == 512, "column band: %s", pass_name(s.pass));
    }
    // N = 4096, one cascade, a band of the context split further by the column passes: for every knob the bands of a
    // unit are contiguous from the context's x0, multiples of 16 wide, and cover the context's band; whatever is
    // left over goes to the last one.  c4_bands lowers the count until it divides the band into multiples of 16, so
    // 3072 columns (192 x 16) take 1..4 and 6 bands as asked, 5 -> 4, 7 -> 6; auto: 4 x 4096 x 3072 x 8 B = 384 MiB
    // -> 2 bands; 2096 columns (131 x 16) only ever one band.
    const int want3072[9] = {2, 1, 2, 3, 4, 4, 6, 6, 8}, want2096[9] = {1, 1, 1, 1, 1, 1, 1, 1, 1};
    for (int nx : {3072, 2096})
        for (int knob = 0; knob <= 8; ++knob) {
            Ctx c(4096, 1, 1);
            c.in.shape.band_x0 = 1024;
            c.in.shape.band_nx = nx;
            c.in.knobs.c4_bands = knob;
            c.finish();
            const Plan p = plan(c, "bands of a band");
            const int nb = (nx == 3072 ? want3072 : want2096)[knob];
            CHECK((int)p.size() == 1 + nb, "band %d knob %d: %zu steps, not %d", nx, knob, p.size(), 1 + nb);
            int x = 1024;
            for (size_t k = 1; k < p.size(); ++k) {
                CHECK(p[k].pass == FramePass::C4Q && p[k].x0 == x && p[k].nx > 0 && p[k].nx % 16 == 0, "band %d knob %d step %zu: [%d, +%d)",
                      nx, knob, k, p[k].x0, p[k].nx);
                x += p[k].nx;
            }
            CHECK(x == 1024 + nx, "band %d knob %d: the bands end at %d", nx, knob, x);
        }
}

void disp_store_policy() {
    struct Case {
        int n, C, T, knob;
        bool want;
        const char* why;
    };
    const Case cases[] = {
        {1024, 4, 1, -1, true, "208 MiB fits"},
        {1024, 4, 1, 0, false, "forced off"},
        {1024, 5, 1, -1, false, "5 x 52 MiB = 260 MiB does not fit (one chunk: 192 / 24 = 8 -> 5 units)"},
        {1024, 5, 1, 1, true, "forced on"},
        {512, 4, 256, 1, false, "more than one chunk"},
        {4096, 4, 1, 1, false, "N > 1024"},
    };
    for (const Case& k : cases) {
        Ctx c(k.n, k.C, k.T);
        c.in.knobs.disp_cached = k.knob;
        for (const FrameStep& s : plan(c, k.why)) CHECK(s.disp_cached == k.want, "disp_cached: %s", k.why);
    }
    Ctx c(1024, 4, 1);  // the four-plane frame never caches DISP
    c.in.knobs.q = 0;
    c.in.knobs.disp_cached = 1;
    for (const FrameStep& s : plan(c, "four-plane frame")) CHECK(!s.disp_cached, "disp_cached: four-plane frame");
}

void stops_at_the_first_failure() {
    Ctx c(512, 4, 256);
    int seen = 0;
    const int r = ocean::plan_frame(c.in, [&](const FrameStep&) { return ++seen == 5 ? 42 : 0; });
    CHECK(r == 42 && seen == 5, "first failure: returned %d after %d steps", r, seen);
}

// the launch counts tests/test_gpu_state.py expects of the library, from the same plans
void gpu_test_shapes() {
    int k0, k1;
    {
        // N 512, C 2, T 3, 12 MiB: K = 2 three-plane units (6 MiB) of 6: three chunks
        Ctx c(512, 2, 3);
        c.in.knobs.chunk_mib = 12;
        c.finish();
        count_kinds(plan(c, "512 x 2 x 3, 12 MiB"), &k0, &k1);
        CHECK(k0 == 3 && k1 == 3, "512 x 2 x 3: %d + %d", k0, k1);
        c.finish({-1, -1, -1, -1, -1, -1});
        count_kinds(plan(c, "512 x 2 x 3, 12 MiB, flat"), &k0, &k1);
        CHECK(k0 == 0 && k1 == 3, "512 x 2 x 3 flat: %d + %d", k0, k1);
    }
    {
        Ctx c(512, 1, 1, 2);
        count_kinds(plan(c, "512 displacement only"), &k0, &k1);
        CHECK(k0 == 1 && k1 == 1, "512 displacement only: %d + %d", k0, k1);
    }
    {
        // N 2048, C 1, T 2, two bands: 128 MiB per unit, K = 1: per unit one row launch and two band launches
        Ctx c(2048, 1, 2);
        c.in.knobs.c4_bands = 2;
        c.finish();
        count_kinds(plan(c, "2048 x 1 x 2, two bands"), &k0, &k1);
        CHECK(k0 == 2 && k1 == 4, "2048 x 1 x 2: %d + %d", k0, k1);
    }
}

}  // namespace

int main(int argc, char**) {
    verbose = argc > 1;
    benchmark_shapes();
    frame_kinds();
    dead_share();
    chunks();
    column_bands();
    disp_store_policy();
    stops_at_the_first_failure();
    gpu_test_shapes();
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
