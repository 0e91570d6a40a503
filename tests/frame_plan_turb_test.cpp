// Stand-alone check of defer_turb (ocean-simulation_amd/csrc/frame_plan.h): which frames leave the TURB array to
// the materialise kernel.  A frame defers only when every column pass of it is pass BQ.  tests/test_frame_plan_turb.py
// builds and runs it; any argument prints every case.
#include <cstdio>
#include <vector>

#include "frame_plan.h"

namespace {

using ocean::FrameInputs;
using ocean::FramePass;
using ocean::FrameStep;

int failures = 0;
bool verbose = false;

// A context as ocean_create and ocean_init_spectrum leave it (default knobs, the spectrum generated, dense extents).
struct Ctx {
    FrameInputs in{};
    ocean::PruneItems prune;
    Ctx(int n, int C, int T, int P = 4) {
        in.shape = {n, C, T, P, 0, 0, n, -1};
        in.knobs = {1, 1, 192, 0, -1, 1};
        in.state = {ocean::pass_a4_supported(n, P), ocean::pass_q_supported(n, P), false, true, false, &prune, false};
        in.state.h0k_valid = in.state.h0k;
        in.shape.inter_units = ocean::inter_units(in);
        const std::vector<int> ext((size_t)T * C, n / 2);
        prune.build(ext.data(), (int)ext.size(), n);
        in.state.prune_ready = ocean::prune_tables(in);
    }
};

// The frame's steps all carry `want`, and a deferring frame has no column pass but pass BQ.
void expect(const Ctx& c, bool want, const char* what) {
    int steps = 0, bq = 0, cols = 0;
    bool same = true;
    ocean::plan_frame(c.in, [&](const FrameStep& s) {
        ++steps;
        same = same && s.defer_turb == want;
        cols += s.kind == 1;
        bq += s.pass == FramePass::B_Q && s.nx == c.in.shape.n;
        return 0;
    });
    const bool ok = steps > 0 && same && ocean::defer_turb(c.in) == want && (!want || bq == cols);
    if (verbose || !ok)
        std::printf("%s %s: defer_turb %d (want %d), %d steps, %d column passes, %d whole-band pass BQ\n", ok ? "ok  " : "FAIL",
                    what, ocean::defer_turb(c.in), want, steps, cols, bq);
    failures += !ok;
}

}  // namespace

int main(int argc, char**) {
    verbose = argc > 1;
    { Ctx c(1024, 4, 1); expect(c, true, "cfg3, 4 x 1024^2"); }
    { Ctx c(512, 4, 256); expect(c, true, "cfg4, 1024 units of 512^2 in chunks"); }
    { Ctx c(512, 2, 1); expect(c, true, "512^2 x 2"); }
    { Ctx c(512, 2, 1); c.in.knobs.defer_turb = 0; expect(c, false, "OCEAN_DEFER_TURB=0"); }
    { Ctx c(512, 2, 1); c.in.state.turb_exposed = true; expect(c, false, "TURB pointer handed out"); }
    { Ctx c(512, 2, 1); c.in.state.h0k_valid = false; c.in.state.h0_conj = false; expect(c, false, "after an H0 upload"); }
    { Ctx c(512, 2, 1); c.in.knobs.q = 0; expect(c, false, "OCEAN_Q=0"); }
    { Ctx c(512, 2, 1); c.in.knobs.a4 = 0; expect(c, false, "OCEAN_A4=0"); }
    { Ctx c(512, 2, 1); c.in.shape.band_x0 = 128; c.in.shape.band_nx = 256; expect(c, false, "column band"); }
    { Ctx c(512, 2, 1, 2); expect(c, false, "displacement only"); }
    { Ctx c(256, 2, 1); expect(c, false, "N = 256"); }
    { Ctx c(2048, 1, 1); expect(c, false, "N = 2048"); }
    { Ctx c(4096, 1, 1); expect(c, false, "N = 4096"); }
    { Ctx c(4096, 1, 1); c.in.shape.col_par = 1; c.in.shape.band_nx = 2048; expect(c, false, "column parity"); }
    if (failures) return 1;
    std::printf("ok\n");
    return 0;
}
