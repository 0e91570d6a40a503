// The schedule of a fused frame (DESIGN.md section 3 "Frame schedule"): host code, no HIP, so that every
// choice below can be read off a printed plan (tests/frame_plan_test.cpp builds it alone).
//
// A frame is a list of timed launches.  plan_frame() walks it in launch order and hands each step to the
// caller; abi_frame.cpp step_fused turns a step into a view of the context and one launch_* call.  What is
// decided here, from the shape, the knobs and a few flags of the context:
//   - three-plane or four-plane frame (use_q, q_planes) and the row pass of the four-plane one;
//   - unit chunks (chunk_units) and where a chunk's intermediate sits (inter_at_base);
//   - column bands of the N >= 2048 column passes (c4_bands);
//   - pass BQ's DISP store policy (disp_fits_cache), and whether it writes TURB at all (defer_turb);
//   - pruned or dense kernels per chunk (prune_pays), and no pass A for a chunk with no live item.
// Per chunk of units: pass A (mirror-pair rows where h0k is valid and the size has them, else per-texel rows),
// then pass B (column tiles, N <= 1024) or the four-step column passes (N >= 2048), those per (unit, column
// band) when a unit has more than one band: pass C2 re-reads what C1 just wrote while it is still in the
// Infinity Cache (256 MiB).
// Both passes of a chunk take the same pruned-or-dense choice.  The choice is per chunk, so dense and pruned
// chunks may alternate over the same intermediate region: a dense pass AQ writes every row its pass BQ reads,
// and a pruned pass BQ reads no row its pass AQ did not write, so neither depends on what the other left there.
// ocean_create sizes the intermediate, h0k, the side arrays and the prune tables with the same functions, so
// the sizing and the schedule cannot drift apart.  Nothing here reads the environment: the knobs arrive as
// values (abi_internal.h ocean_options::from_env).
#pragma once

#include <algorithm>
#include <cstddef>

#include "prune_items.h"

namespace ocean {

struct FrameShape {
    int n, C, T, P;        // grid side, cascades, tiles, planes (4 full, 2 displacement only)
    size_t inter_units;    // units the intermediate holds (0 while ocean_create sizes it)
    int band_x0, band_nx;  // column band of the fused passes; nx = n: whole
    int col_par;           // column parity: -1 off
};
struct FrameKnobs {
    int q, a4;        // OCEAN_Q, OCEAN_A4
    long chunk_mib;   // OCEAN_CHUNK_MIB
    int c4_bands;     // OCEAN_C4_BANDS, 0 = auto
    int disp_cached;  // OCEAN_DISP_CACHED, -1 = auto
    int defer_turb;   // OCEAN_DEFER_TURB: 0 = every frame writes TURB
};
struct FrameState {
    bool h0k, qside;    // allocated
    bool h0k_valid;     // h0k matches h0
    bool h0_conj;       // h0.zw = conj h0(-k)
    bool prune_ready;   // `prune` was built from the spectrum in h0k
    const PruneItems* prune;
    bool turb_exposed;  // ocean_get_device_ptr has handed TURB out: every frame writes it
};
struct FrameInputs {
    FrameShape shape;
    FrameKnobs knobs;
    FrameState state;
    int units() const { return shape.T * shape.C; }
    size_t texels() const { return (size_t)shape.n * shape.n; }
};

// fft4k.hip: the four-step column passes replace pass B
inline bool pass_c4_supported(int n) { return n == 2048 || n == 4096; }
// fft3.hip, the mirror-pair row pass: N = 512 / 1024 with four planes; N = 256 / 512 displacement-only (two planes)
inline bool pass_a4_supported(int n, int planes) {
    if (planes == 2) return n == 256 || n == 512;
    return planes == 4 && (n == 512 || n == 1024);
}
// fftq.hip, the three-plane frame.  N = 2048 keeps the four-plane passes: pass A3Q's idle fourth sequence slot
// costs more there than the column passes save (4 x 2048^2: 612 against 599 us per frame; docs/MEASUREMENTS.md
// section 3).
inline bool pass_q_supported(int n, int planes) { return planes == 4 && (n == 512 || n == 1024 || n == 4096); }
// intermediate planes of the three-plane frame: Q1..Q3, plus the four-step column passes' R[Q4]
inline int q_planes(int n) { return n >= 2048 ? 4 : 3; }

// Units per chunk: a frame over many units runs pass A and pass B chunk by chunk so
// that the intermediate pass B re-reads is still in the 256 MiB Infinity Cache
// (OCEAN_CHUNK_MIB of intermediate per chunk, 0 = whole frame at once; a unit larger than a
// chunk: whole frame).  Measured on cfg4's 1024 units at 512^2 (8 MiB each): 64 MiB 37.9k,
// 128 MiB 40.7k, 192 MiB 43.1k, 256 MiB 38.4k, unchunked 40.7k tile-frames/s.
inline int chunk_units(const FrameInputs& in, int planes) {
    const long mib = in.knobs.chunk_mib;
    const int U = in.units();
    if (mib <= 0) return U;
    const size_t per_unit = in.texels() * 8 * planes;
    int k = (int)(((size_t)mib << 20) / per_unit);
    if (k >= in.shape.C) k -= k % in.shape.C;  // whole tiles when a chunk holds one
    if (k < 1) return U;
    return k >= U ? U : k;
}
// Units of the intermediate: a chunk of either schedule, P planes, or (three-plane frame) planes Q1..Q3 plus
// the per-unit side arrays in the fourth plane's room (fftq.hip).
inline size_t inter_units(const FrameInputs& in) {
    const FrameShape& sh = in.shape;
    return (size_t)std::max(chunk_units(in, sh.P), pass_q_supported(sh.n, sh.P) ? chunk_units(in, q_planes(sh.n)) : 1);
}

// Column bands per unit for the N >= 2048 column passes: OCEAN_C4_BANDS, or by default
// as many as keep one band's planes (P * N * width * 8 B) within 256 MiB -- cfg5's 512 MiB
// units run as 2 bands: 387 -> 412-421 frames/s (3 or 4 bands: 417; per-unit pass A: slower).
// Band widths stay multiples of the four-step tile width (16).
inline int c4_bands(const FrameInputs& in, int nx) {
    if (!pass_c4_supported(in.shape.n)) return 1;
    int nb = in.knobs.c4_bands;
    if (nb <= 0) {
        const size_t band_bytes = (size_t)in.shape.P * in.shape.n * nx * 8;
        nb = 1;
        while (band_bytes / nb > ((size_t)256 << 20)) nb *= 2;
    }
    while (nb > 1 && (nx % nb || (nx / nb) % 16)) --nb;
    return nb;
}

// The three-plane fused frame (fftq.hip) runs where it applies: N = 512 / 1024 with full
// outputs, the mirror-pair row pass's h0k valid.
inline bool use_q(const FrameInputs& in) {
    if (!in.knobs.q || !in.state.h0_conj || !pass_q_supported(in.shape.n, in.shape.P)) return false;
    return in.shape.n >= 2048 || (in.knobs.a4 && in.state.h0k_valid);  // N <= 1024: the mirror-pair row pass reads h0k
}

// Pass BQ may write DISP with default-policy stores (DevView::disp_cached) when the whole frame is one chunk
// and its cache-resident set plus DISP fits 224 MiB of the 256 MiB Infinity Cache of an MI355X: DISP then
// waits there and is written back while the next pass A runs, when HBM has headroom.  The resident set is
// what the three-plane frame re-reads each frame, per texel-cascade: pass AQ's h0k (8 B; the frame runs
// only with the mirror-pair row pass, use_q), the intermediate Q1..Q3 (24 B) and the foam state (4 B).
// cfg3 (4 x 1024^2, 208 MiB): 11.83-11.88 -> 12.08-12.11 k frames/s; a cfg4 chunk (32 units of 512^2,
// 288 MiB) lost 7.5 % the same way, and DISP + TURB at cfg3 lost 7 % (docs/MEASUREMENTS.md section 8).
// The 224 MiB budget is this part's; OCEAN_DISP_CACHED=0 / 1 overrides the choice (A/B, other parts).
inline bool disp_fits_cache(const FrameInputs& in, bool q, int chunk) {
    if (!q || in.shape.n > 1024 || chunk < in.units()) return false;
    if (in.knobs.disp_cached >= 0) return in.knobs.disp_cached != 0;
    constexpr size_t kH0k = 8, kInter = 24, kFoam = 4, kDisp = 16;
    const size_t bytes = in.texels() * in.units() * (kH0k + kInter + kFoam + kDisp);
    return bytes <= ((size_t)224 << 20);
}

// Deferred TURB: TURB is the broadcast RGBA image of the foam state, 16 B per texel-cascade written to carry
// the 4 B that pass BQ stores one line earlier, and every consumer inside the library reads .x alone.  A frame
// whose column passes are all k_pass_bq (N = 512 / 1024, three-plane, whole column band, no parity) may leave the
// float4 array as it is: the foam state is then TURB's level 0, the point consumers tap it (sample_filter.h), and
// the entries that show the array itself materialise it first (abi_context.cpp materialise_turb).  Never deferred:
// four-plane frames (after an H0 upload, OCEAN_Q=0, OCEAN_A4=0), N >= 2048, bands and parities, and a context
// whose TURB pointer ocean_get_device_ptr has handed out.  Unfused and displacement-only contexts plan no such
// frame (P = 2 fails pass_q_supported; ocean_step does not plan an unfused one).
inline bool defer_turb(const FrameInputs& in) {
    if (!in.knobs.defer_turb || in.state.turb_exposed) return false;
    if (in.shape.n > 1024 || in.shape.band_nx != in.shape.n || in.shape.col_par >= 0) return false;
    return use_q(in);
}

// Band-limited cascades: a context keeps live extents and an item table (prune_items.h) where passes AQ / BQ
// can run pruned: the side arrays and h0k exist, N <= 1024, and a unit index fits the packed item.
inline bool prune_tables(const FrameInputs& in) {
    return in.state.qside && in.state.h0k && in.shape.n <= 1024 && in.units() < kPruneMaxUnits;
}
// The pruned kernels measured 2.2 % of a frame slower than the dense ones where 1.8 % of the items are dead
// (a scene whose amplitudes underflow in a few outer rows) and 4.7-6.6 % faster where 22 % are
// (docs/MEASUREMENTS.md section 13); in between nothing is measured.  A chunk runs them when at least
// 1 / kPruneMinDeadShare of its items is dead, else (a fully dense context included) the dense kernels.
constexpr long kPruneMinDeadShare = 8;
inline bool prune_pays(long live_items, long dense_items) {
    return live_items * kPruneMinDeadShare <= dense_items * (kPruneMinDeadShare - 1);
}

enum class FramePass { A_Q, A_V4, A_V3, B_Q, B_V3, C4, C4Q };

// One timed launch of a frame.
struct FrameStep {
    FramePass pass;
    int kind;            // kernel-timing kind: 0 the row pass, 1 the column pass(es)
    const char* name;    // of the timed call (the text of a launch failure)
    int u0, nu;          // units [u0, u0 + nu) of the context
    bool inter_at_base;  // the chunk's intermediate starts at the base of every plane (one region reused by
                         // every chunk), else every unit keeps its own slot
    int inter_u0;        // unit slot of the intermediate (and of the side arrays) that holds unit u0
    int x0, nx;          // column band
    bool disp_cached;    // DevView::disp_cached
    bool pruned;         // passes AQ / BQ over the live rows: items [first, first + items) of the table are the
    int first, items, ubase;  // step's, and its unit 0 is context unit ubase
    bool defer_turb;     // DevView::turb_defer: pass BQ stores no TURB (the same for every step of a frame)
};

// Calls step(const FrameStep&) once per timed launch of the frame, in launch order; stops at the first non-zero
// return and returns it.  No allocation: small jobs issue a frame every few microseconds.
template <class F>
int plan_frame(const FrameInputs& in, F&& step) {
    const FrameShape& sh = in.shape;
    const bool q = use_q(in), c4 = pass_c4_supported(sh.n);
    // h0k also exists at 4096 (pass A3PP), where the mirror-pair pass A4 does not
    const bool a4 = in.knobs.a4 && in.state.h0k_valid && pass_a4_supported(sh.n, sh.P);
    const int U = in.units(), K = std::min(chunk_units(in, q ? q_planes(sh.n) : sh.P), (int)sh.inter_units);
    const int nb = c4_bands(in, sh.band_nx), w = sh.band_nx / nb;
    const bool at_base = sh.inter_units < (size_t)U, prunable = q && !c4 && in.state.prune_ready && !in.state.prune->dense;
    for (int u0 = 0; u0 < U; u0 += K) {
        const int nu = std::min(K, U - u0), slot = at_base ? 0 : u0;
        FrameStep st{q ? FramePass::A_Q : a4 ? FramePass::A_V4 : FramePass::A_V3, 0, "pass_a", u0, nu, at_base, slot,
                     sh.band_x0, sh.band_nx, disp_fits_cache(in, q, K), prunable && sh.band_nx == sh.n, 0, 0, u0,
                     defer_turb(in)};
        if (st.pruned) {
            in.state.prune->chunk(u0, nu, &st.first, &st.items);
            st.pruned = prune_pays(st.items, (long)nu * (sh.n / 2 + 1));
        }
        if (!st.pruned || st.items > 0)  // a chunk with no live item launches no pass A
            if (int r = step(st)) return r;
        st.kind = 1;
        st.pass = !c4 ? (q ? FramePass::B_Q : FramePass::B_V3) : (q ? FramePass::C4Q : FramePass::C4);
        st.name = c4 && (q || nb > 1) ? "pass_c" : "pass_b";  // (the names the two frames have always reported)
        if (nb == 1) {  // N <= 1024, or one band: the chunk at once
            if (int r = step(st)) return r;
            continue;
        }
        st.nu = 1;
        for (int u = 0; u < nu; ++u)
            for (int b = 0; b < nb; ++b) {
                st.u0 = u0 + u;
                st.inter_u0 = slot + u;
                st.x0 = sh.band_x0 + b * w;
                st.nx = (b == nb - 1) ? sh.band_nx - b * w : w;
                if (int r = step(st)) return r;
            }
    }
    return 0;
}

}  // namespace ocean
