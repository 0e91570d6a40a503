// C-ABI layer of liboceanhip.so, the frame: the step and its stages, the fused frame's launches from its plan
// (frame_plan.h), the surface velocity, and kernel timing.
#include <cxxabi.h>

#include <cstdio>

#include "abi_internal.h"

// Folds timed launches into kind_ms / kind_count and returns their events to the pool.
// wait: synchronize the stream first (every pending launch is then finished); else fold
// the finished prefix only (stream order: the first unfinished launch ends it).
int fold_pending(ocean_ctx* ctx, bool wait) {
    if (wait) OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    size_t k = 0;
    for (; k < ctx->pending.size(); ++k) {
        const TimedLaunch& t = ctx->pending[k];
        if (!wait) {
            const hipError_t q = hipEventQuery(t.b);
            if (q == hipErrorNotReady) break;
            if (q != hipSuccess) return hip_fail(q, "hipEventQuery");
        }
        float ms = 0.0f;
        OCEAN_HIP(hipEventElapsedTime(&ms, t.a, t.b));
        ctx->kind_ms[t.kind] += ms;
        ctx->kind_count[t.kind] += 1;
        ctx->event_pool.push_back(t.a);
        ctx->event_pool.push_back(t.b);
    }
    ctx->pending.erase(ctx->pending.begin(), ctx->pending.begin() + k);
    return OCEAN_OK;
}

extern "C" {

int ocean_evolve(ocean_ctx* ctx, float time) {
    OCEAN_ENTER(ctx);
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_evolve");
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2, [&] { return ocean::launch_evolve(v, time, ctx->stream); }, "evolve");
}

namespace {
// The operator IFFT over `ups` consecutive unit-planes from `base`, in place; its row launches are timed as
// kind `kind_rows`, its column launches as `kind_cols`.
int ifft_unit_planes(ocean_ctx* ctx, const ocean::DevView& v, float2* base0, int ups, int kind_rows, int kind_cols) {
    const size_t up_elems = ctx->texels();  // one unit-plane
    // In-place row and column launches per chunk of at most OCEAN_OP_CHUNK_MIB of unit-planes, so
    // the column launch re-reads the rows' output from the Infinity Cache when the plane set is
    // larger than it.  Auto: 256 MiB (4 x 4 x 1024^2 x 4 planes, 512 MiB, fresh data: 128 / 192 /
    // 256 / 320 / 384 MiB / unchunked 0.69 / 0.69 / 0.736 / 0.63 / 0.60 / 0.57 of peak; cfg3's 128
    // MiB: one chunk; at N = 4096 two unit-planes, docs/MEASUREMENTS.md section 8).  At N = 1024 / 2048
    // the column launch takes XCD-paired halves of 16-column tiles (fft2.hip Cols2).
    // N = 4096: folded columns (fft2.hip k_rowsf / k_colsf_ip): rows + the decimation-in-frequency fold
    // onto the planes' own rows (z_b at rows b L + n), then 2048-point column tiles of both sub-planes
    // per item, back into the planes, permuted.
    const bool fold = ctx->n == 4096;
    const hipStream_t s = ctx->stream;
    const long mib = ctx->opt.op_chunk_mib > 0 ? ctx->opt.op_chunk_mib : 256;
    const int k = (int)std::max<size_t>(1, ((size_t)mib << 20) / (up_elems * 8));
    for (int c0 = 0; c0 < ups; c0 += k) {
        const int kc = std::min(k, ups - c0);
        float2* base = base0 + (size_t)c0 * up_elems;
        auto rows = [&] { return fold ? ocean::launch_ifft_fold(v, base, kc, 0, s) : ocean::launch_ifft_rows_v2(v, base, kc, s); };
        auto cols = [&] { return fold ? ocean::launch_ifft_fold(v, base, kc, 1, s) : ocean::launch_ifft_cols_v2(v, base, kc, s); };
        if (int r = timed(ctx, kind_rows, rows, "ifft_rows")) return r;
        if (int r = timed(ctx, kind_cols, cols, "ifft_cols")) return r;
    }
    return OCEAN_OK;
}
}  // namespace

int ocean_ifft2d(ocean_ctx* ctx, int plane_mask) {
    OCEAN_ENTER(ctx);
    if (plane_mask < 0 || plane_mask > 15) return fail(OCEAN_E_INVALID_ARG, "plane_mask must be in [0, 15]");
    for (int p = 0; p < 4; ++p)
        if ((plane_mask & (1 << p)) && p >= ctx->P)
            return fail(OCEAN_E_INVALID_ARG, "plane not allocated (DISPLACEMENT_ONLY context)");
    const ocean::DevView v = ctx->view();
    for (int p = 0; p < 4;) {
        if (!(plane_mask & (1 << p))) {
            ++p;
            continue;
        }
        int np = 1;  // run of consecutive planes: one launch per direction (planes are one allocation)
        while (p + np < 4 && (plane_mask & (1 << (p + np)))) ++np;
        if (int r = ifft_unit_planes(ctx, v, ctx->plane[p], np * (int)ctx->units(), 0, 1)) return r;
        p += np;
    }
    return OCEAN_OK;
}

int ocean_fill(ocean_ctx* ctx) {
    OCEAN_ENTER(ctx);
    drop_bounds(ctx);
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2, [&] { return ocean::launch_fill(v, ctx->stream); }, "fill")) return r;
    if (ctx->P == 4) ctx->turb_stale = false;  // deferred TURB: the fill wrote every texel of TURB from the foam state
    return OCEAN_OK;
}

namespace {
int step_fused(ocean_ctx* ctx, float time);

// GenerateMips (WaterBody.cs:191-192) when the context has mip chains.
int generate_mips(ocean_ctx* ctx) {
    if (!(ctx->flags & OCEAN_F_MIPS)) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2, [&] { return ocean::launch_mips(v, ctx->stream); }, "mips");
}

// OCEAN_F_VELOCITY: VEL at `time`, after the frame on the ctx stream (ocean.h): dh/dt packed into the two
// scratch planes, the operator IFFT over them as 2 U unit-planes (chunked like ocean_ifft2d), interleaved
// into VEL.  Every launch is kind 2: kinds 0 and 1 stay the frame's two passes.
int step_velocity(ocean_ctx* ctx, float time) {
    if (!(ctx->flags & OCEAN_F_VELOCITY)) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2, [&] { return ocean::launch_evolve_velocity(v, ctx->vplane, time, ctx->stream); },
                      "evolve_velocity"))
        return r;
    if (int r = ifft_unit_planes(ctx, v, ctx->vplane, 2 * (int)ctx->units(), 2, 2)) return r;
    return timed(ctx, 2,
                 [&] { return ocean::launch_pack_velocity(v, ctx->vplane, ctx->vel, ctx->opt.vel_nt != 0, ctx->stream); },
                 "pack_velocity");
}
}  // namespace

int ocean_step(ocean_ctx* ctx, float time) {
    OCEAN_ENTER(ctx);
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_step");
    drop_bounds(ctx);
    if (ctx->flags & OCEAN_F_UNFUSED) {
        if (int r = ocean_evolve(ctx, time)) return r;
        if (int r = ocean_ifft2d(ctx, (1 << ctx->P) - 1)) return r;
        if (int r = ocean_fill(ctx)) return r;
    } else {
        if (int r = step_fused(ctx, time)) return r;
    }
    if (int r = generate_mips(ctx)) return r;
    return step_velocity(ctx, time);
}

namespace {
// View of units [u0, u0 + nu) (unit u of the view is cascade (c0 + u) % C), whose intermediate and side arrays
// start at unit slot inter_u0 (FrameStep::inter_u0).
ocean::DevView sub_view(const ocean::DevView& v, int u0, int nu, int inter_u0) {
    ocean::DevView s = v;
    const size_t off = (size_t)u0 * v.n * v.n;
    s.units = nu;
    s.c0 = (v.c0 + u0) % v.C;
    s.h0 = v.h0 + off;
    s.waves = v.waves + off;
    if (v.h0k) s.h0k = v.h0k + off;
    // plane_stride unchanged: planes stay U * N * N apart
    s.tplane = v.tplane + (size_t)inter_u0 * v.n * v.n;
    if (v.foam) s.foam = v.foam + off;
    if (v.qside) s.qside = v.qside + (size_t)inter_u0 * 2 * v.n;
    s.disp = v.disp + off;
    if (v.deriv) s.deriv = v.deriv + off;
    if (v.turb) s.turb = v.turb + off;
    if (v.normal) s.normal = v.normal + off;
    return s;
}

// One frame: the steps of its plan (frame_plan.h), each a view of its units and column band and one launch.
int step_fused(ocean_ctx* ctx, float time) {
    ocean::DevView v = ctx->view();
    if (!ctx->h0k_valid) v.h0k = nullptr;  // stale after an H0 upload: no row pass may read it
    const ocean::FrameInputs in = ctx->frame_inputs();
    if (ctx->col_par >= 0 && !ocean::use_q(in))
        return fail(OCEAN_E_STATE, "a column parity needs the three-plane frame (h0 from ocean_init_spectrum)");
    const hipStream_t s = ctx->stream;
    // deferred TURB: a deferred frame leaves the float4 array stale; a frame that writes TURB starts from a whole
    // array (it may write a part of it only), which costs a launch on the first such frame after deferred ones
    if (ocean::defer_turb(in)) ctx->turb_stale = true;
    else if (int r = materialise_turb(ctx)) return r;
    return ocean::plan_frame(in, [&](const ocean::FrameStep& st) {
        ocean::DevView c = sub_view(v, st.u0, st.nu, st.inter_u0);
        c.x0 = st.x0;
        c.nx = st.nx;
        c.disp_cached = st.disp_cached;
        c.turb_defer = st.defer_turb;
        // band-limited cascades: the step's live items and the extents of its units
        ocean::PruneView pv{};
        if (st.pruned) pv = {ctx->prune_dev + ctx->units() + st.first, st.items, st.ubase, ctx->prune_dev + st.u0};
        const ocean::PruneView* pp = st.pruned ? &pv : nullptr;
        return timed(ctx, st.kind, [&] {
            switch (st.pass) {
                case ocean::FramePass::A_Q: return ocean::launch_pass_a_q(c, time, s, pp);
                case ocean::FramePass::A_V4: return ocean::launch_pass_a_v4(c, time, s);
                case ocean::FramePass::A_V3: return ocean::launch_pass_a_v3(c, time, s);
                case ocean::FramePass::B_Q: return ocean::launch_pass_b_q(c, s, pp);
                case ocean::FramePass::B_V3: return ocean::launch_pass_b_v3(c, s);
                case ocean::FramePass::C4: return ocean::launch_pass_c4(c, s);
                case ocean::FramePass::C4Q: return ocean::launch_pass_c4q(c, s);
            }
            return hipErrorInvalidValue;
        }, st.name);
    });
}
}  // namespace

int ocean_set_kernel_timing(ocean_ctx* ctx, int enable) {
    OCEAN_ENTER(ctx);
    if (enable && ctx->event_pool.size() < 4096) {
        // pre-create events so the timed region never creates any
        while (ctx->event_pool.size() < 4096) {
            hipEvent_t e = nullptr;
            OCEAN_HIP(hipEventCreate(&e));
            ctx->event_pool.push_back(e);
        }
    }
    if (!enable && !ctx->pending.empty())  // launches timed so far still count at the next ocean_kernel_stats
        if (int r = fold_pending(ctx, true)) return r;
    ctx->timing = enable != 0;
    return OCEAN_OK;
}

int ocean_step_bytes(ocean_ctx* ctx, uint64_t* pass_a, uint64_t* pass_b) {
    if (!ctx || !pass_a || !pass_b) return fail(OCEAN_E_INVALID_ARG, "null argument");
    const uint64_t tex = (uint64_t)ctx->texels() * ctx->units();
    const uint64_t P = ctx->P;
    const bool full = P == 4, normals = (ctx->flags & OCEAN_F_NORMALS) != 0;
    const uint64_t outs = 16 + (full ? 32 : 0) + (normals ? 16 : 0);  // DISP [+ DERIV + TURB] [+ NORMAL]
    uint64_t a = 0, b = 0;
    if (ctx->flags & OCEAN_F_UNFUSED) {
        // evolve: h0 + waves -> P planes; rows and columns: read + write every plane;
        // fill: P planes [+ foam state read + write] -> outputs
        a = tex * (32 + 8 * P + 16 * P);
        b = tex * (16 * P + 8 * P + (full ? 8 : 0) + outs);
    } else {
        const bool a4 = ctx->opt.a4 && ctx->h0k_valid && ocean::pass_a4_supported(ctx->n, ctx->P);
        // column band: h0 is read whole (rows are transformed whole), the rest scales with the band
        const uint64_t bt = tex / ctx->n * ctx->band_nx;
        if (ocean::use_q(ctx->frame_inputs())) {
            // three-plane frame (the side arrays, 16 B per row, not counted): pass A h0k (h0 at
            // N >= 2048) -> Q1..Q3; pass B Q1..Q3 + foam state -> outputs, or at N >= 2048 the
            // four-step passes: C1 reads Q1..Q3 and writes them with R[Q4], C2 reads four planes
            // the column-parity row pass on mirror-pair rows (pass A3PP) reads h0k, 8 B per texel
            const bool h0k_pairs = ctx->col_par >= 0;
            *pass_a = tex * ((ctx->n >= 2048 && !h0k_pairs) ? 16 : 8) + bt * 24;
            *pass_b = ctx->n >= 2048 ? bt * (24 + 32 + 32 + 8 + outs) : bt * (24 + 8 + outs);
            return OCEAN_OK;
        }
        a = tex * (a4 ? 8 : 16) + bt * 8 * P;
        b = bt * (8 * P + (full ? 8 : 0) + outs);  // + foam state read and write
        if (ocean::pass_c4_supported(ctx->n)) b += bt * 16 * P;  // four-step: step 1 reads + writes the planes
    }
    *pass_a = a;
    *pass_b = b;
    return OCEAN_OK;
}

int ocean_kernel_name(ocean_ctx* ctx, int kind, char* buf, size_t len) {
    if (!ctx || !buf || len == 0) return fail(OCEAN_E_INVALID_ARG, "null argument or zero length");
    if (kind < 0 || kind > 2) return fail(OCEAN_E_INVALID_ARG, "bad kind");
    buf[0] = 0;
    if (!ctx->kind_kernel[kind]) return fail(OCEAN_E_STATE, "no kernel of this kind launched yet");
    OCEAN_ENTER(ctx);
    const char* mangled = hipKernelNameRefByPtr(ctx->kind_kernel[kind], ctx->stream);
    if (!mangled) return fail(OCEAN_E_DEVICE, "hipKernelNameRefByPtr returned no name");
    int st = 0;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &st);
    const std::string name = (st == 0 && dem) ? dem : mangled;
    std::free(dem);
    std::snprintf(buf, len, "%s", name.c_str());
    return name.size() < len ? OCEAN_OK : fail(OCEAN_E_INVALID_ARG, "buffer too small for " + name);
}

int ocean_kernel_stats(ocean_ctx* ctx, int kind, double* total_ms, long long* launches) {
    OCEAN_ENTER(ctx);
    if (kind < 0 || kind > 2 || !total_ms || !launches) return fail(OCEAN_E_INVALID_ARG, "bad kind or null output");
    if (int r = fold_pending(ctx, true)) return r;
    *total_ms = ctx->kind_ms[kind];
    *launches = ctx->kind_count[kind];
    ctx->kind_ms[kind] = 0;
    ctx->kind_count[kind] = 0;
    return OCEAN_OK;
}

}  // extern "C"
