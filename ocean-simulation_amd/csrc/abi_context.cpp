// C-ABI layer of liboceanhip.so, the context: its lifetime, parameters, noise and initial spectrum, the texture
// reads, writes and device pointers, and the column band and parity of a shard.  See include/ocean/ocean.h for
// the reference interface each entry point replaces.
#include <cmath>
#include <new>

#include "abi_internal.h"
#include "fft_core.h"

namespace {
thread_local std::string g_last_error;
}

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(OCEAN_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

// Host noise generator (WaterBody.cs:71-100 with this library's documented
// uniform source).  Defined in noise.cpp.
namespace ocean {
void generate_noise_host(int n, uint64_t seed, float* out);
}

namespace {

void* tex_ptr(ocean_ctx* ctx, int tex, size_t* elem_bytes, size_t* slices) {
    *slices = ctx->units();
    switch (tex) {
        case OCEAN_TEX_NOISE: *elem_bytes = 8; *slices = ctx->T; return ctx->noise;
        case OCEAN_TEX_H0: *elem_bytes = 16; return ctx->h0;
        case OCEAN_TEX_WAVES: *elem_bytes = 16; return ctx->waves;
        case OCEAN_TEX_PLANE0:
        case OCEAN_TEX_PLANE1:
        case OCEAN_TEX_PLANE2:
        case OCEAN_TEX_PLANE3: *elem_bytes = 8; return ctx->plane[tex - OCEAN_TEX_PLANE0];
        case OCEAN_TEX_DISP: *elem_bytes = 16; return ctx->disp;
        case OCEAN_TEX_DERIV: *elem_bytes = 16; return ctx->deriv;
        case OCEAN_TEX_TURB: *elem_bytes = 16; return ctx->turb;
        case OCEAN_TEX_NORMAL: *elem_bytes = 16; return ctx->normal;
        case OCEAN_TEX_VELOCITY: *elem_bytes = 16; return ctx->vel;
    }
    return nullptr;
}

}  // namespace

int materialise_turb(ocean_ctx* ctx) {
    if (!ctx->turb_stale) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2, [&] { return ocean::launch_turb_materialise(v, ctx->stream); }, "turb_materialise"))
        return r;
    ctx->turb_stale = false;
    return OCEAN_OK;
}

int slice_ptr(ocean_ctx* ctx, int tex, int tile, int cascade, size_t bytes, char** out) {
    size_t eb = 0, slices = 0;
    void* base = tex_ptr(ctx, tex, &eb, &slices);
    if (tex < OCEAN_TEX_NOISE || tex > OCEAN_TEX_VELOCITY) return fail(OCEAN_E_INVALID_ARG, "unknown texture id");
    if (!base) return fail(OCEAN_E_INVALID_ARG, "texture not allocated for this context's flags");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    if (tex != OCEAN_TEX_NOISE && (cascade < 0 || cascade >= ctx->C))
        return fail(OCEAN_E_INVALID_ARG, "cascade out of range");
    const size_t slice_bytes = ctx->texels() * eb;
    if (bytes != slice_bytes)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != slice size " +
                                             std::to_string(slice_bytes));
    const size_t slice = tex == OCEAN_TEX_NOISE ? (size_t)tile : (size_t)tile * ctx->C + cascade;
    *out = static_cast<char*>(base) + slice * slice_bytes;
    return OCEAN_OK;
}

namespace {

void free_all(ocean_ctx* c) {
    void* ptrs[] = {c->noise, c->h0, c->h0k, c->waves, c->plane[0], c->disp, c->deriv,
                    c->turb,  c->normal, c->tw,    c->casc,     c->tplane, c->foam, c->deriv_mips, c->turb_mips,
                    c->qside, c->vel, c->vplane, c->prune_dev, c->bounds_dev.ptr, c->whitecap_dev.ptr, c->spray_dev.ptr,
                    c->stage_block, c->atm.block};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    for (auto& t : c->pending) {
        (void)hipEventDestroy(t.a);
        (void)hipEventDestroy(t.b);
    }
    for (auto e : c->event_pool) (void)hipEventDestroy(e);
    if (c->copy_stream) (void)hipStreamDestroy(c->copy_stream);
    if (c->stream) (void)hipStreamDestroy(c->stream);
}

}  // namespace

extern "C" {

const char* ocean_last_error(void) { return g_last_error.c_str(); }

int ocean_abi_version(void) { return OCEAN_ABI_VERSION; }

int ocean_create(int device, int n, int n_cascades, int n_tiles, uint32_t flags, ocean_ctx** out) {
    g_last_error.clear();
    if (!out) return fail(OCEAN_E_INVALID_ARG, "out is null");
    *out = nullptr;
    if (n < 16 || n > 4096 || (n & (n - 1)) != 0)
        return fail(OCEAN_E_UNSUPPORTED, "n must be a power of two in [16, 4096], got " + std::to_string(n));
    if (n_cascades < 1 || n_cascades > ocean::kMaxCascades)
        return fail(OCEAN_E_UNSUPPORTED, "n_cascades must be in [1, 5], got " + std::to_string(n_cascades));
    if (n_tiles < 1) return fail(OCEAN_E_INVALID_ARG, "n_tiles must be >= 1");
    if (flags & ~(OCEAN_F_DISPLACEMENT_ONLY | OCEAN_F_NORMALS | OCEAN_F_UNFUSED | OCEAN_F_MIPS | OCEAN_F_VELOCITY))
        return fail(OCEAN_E_INVALID_ARG, "unknown flag bits");
    if ((flags & OCEAN_F_DISPLACEMENT_ONLY) && (flags & OCEAN_F_NORMALS))
        return fail(OCEAN_E_INVALID_ARG, "NORMALS needs the derivative planes (not DISPLACEMENT_ONLY)");
    if ((flags & OCEAN_F_DISPLACEMENT_ONLY) && (flags & OCEAN_F_MIPS))
        return fail(OCEAN_E_INVALID_ARG, "MIPS chains are on DERIV and TURB (not DISPLACEMENT_ONLY)");
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess) return hip_fail(e, "hipGetDeviceCount");
    if (device < 0 || device >= ndev) return fail(OCEAN_E_INVALID_ARG, "device index out of range");
    DeviceScope device_scope(device);  // the caller's current device is restored on return
    if (const int r = device_scope.status()) return r;

    ocean_ctx* c = new (std::nothrow) ocean_ctx();
    if (!c) return fail(OCEAN_E_OUT_OF_MEMORY, "host allocation failed");
    c->device = device;
    c->n = n;
    c->logn = 0;
    while ((1 << c->logn) < n) c->logn++;
    c->C = n_cascades;
    c->T = n_tiles;
    c->flags = flags;
    c->P = (flags & OCEAN_F_DISPLACEMENT_ONLY) ? 2 : 4;
    c->noise_set.assign(n_tiles, false);
    c->bounds_valid.assign(n_tiles, false);
    c->band_nx = n;
    c->opt = ocean_options::from_env();
    // Width of the fused path's column tiles.  With fewer tiles than CUs (one 512^2
    // cascade: 32 tiles of 16 columns) pass B ran on an eighth of the chip, so small
    // jobs at N <= 512 take 4-column tiles (docs/MEASUREMENTS.md section 3; at N = 1024 pass A's
    // 32-byte tile rows cost what pass B gains).  OCEAN_TILE_W overrides (A/B).
    c->tile_w = ocean::fftcore::inter_w(n);
    {
        int cus = 256;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess || cus <= 0)
            cus = 256;
        const long tiles = (long)n_cascades * n_tiles * (n / c->tile_w);
        if (n >= 128 && n <= 512 && tiles < cus) c->tile_w = 4;
        const int w = c->opt.tile_w;
        if (w && n >= 128 && n <= 1024 && (w == 4 || w == ocean::fftcore::inter_w(n))) c->tile_w = w;
    }

    auto alloc = [&](void** p, size_t bytes) -> bool {
        if (hipMalloc(p, bytes) != hipSuccess) return false;
        return hipMemset(*p, 0, bytes) == hipSuccess;
    };
    const size_t tex = c->texels(), U = c->units();
    bool ok = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) == hipSuccess;
    ok = ok && alloc((void**)&c->noise, tex * c->T * 8);
    ok = ok && alloc((void**)&c->h0, tex * U * 16);
    // h0k: the mirror-pair row passes (N = 256 / 512 / 1024; at 4096 the column-parity pass A3PP allocates
    // it in ocean_set_column_parity)
    if (ocean::pass_a4_supported(n, c->P)) ok = ok && alloc((void**)&c->h0k, tex * U * 8);
    ok = ok && alloc((void**)&c->waves, tex * U * 16);
    ok = ok && alloc((void**)&c->plane[0], tex * U * 8 * c->P);  // planes contiguous (one descriptor in pass A)
    if (ok)
        for (int p = 1; p < c->P; ++p) c->plane[p] = c->plane[0] + (size_t)p * tex * U;
    ok = ok && alloc((void**)&c->disp, tex * U * 16);
    if (c->P == 4) {
        ok = ok && alloc((void**)&c->deriv, tex * U * 16);
        ok = ok && alloc((void**)&c->turb, tex * U * 16);
        ok = ok && alloc((void**)&c->foam, tex * U * 4);
    }
    // the intermediate holds a chunk of either schedule (frame_plan.h)
    c->inter_units = ocean::inter_units(c->frame_inputs());
    ok = ok && alloc((void**)&c->tplane, tex * c->inter_units * 8 * c->P);
    if (ocean::pass_q_supported(n, c->P)) ok = ok && alloc((void**)&c->qside, c->inter_units * 2 * n * 8);
    if (c->opt.prune && ocean::prune_tables(c->frame_inputs()))
        ok = ok && alloc((void**)&c->prune_dev, (U + U * (n / 2 + 1)) * sizeof(int));
    if (flags & OCEAN_F_NORMALS) ok = ok && alloc((void**)&c->normal, tex * U * 16);
    if (flags & OCEAN_F_MIPS) {
        for (int l = 1; (n >> l) >= 1; ++l) c->mip_chain += (size_t)(n >> l) * (n >> l);
        ok = ok && alloc((void**)&c->deriv_mips, c->mip_chain * U * 16);
        ok = ok && alloc((void**)&c->turb_mips, c->mip_chain * U * 16);
    }
    if (flags & OCEAN_F_VELOCITY) {
        ok = ok && alloc((void**)&c->vel, tex * U * 16);
        ok = ok && alloc((void**)&c->vplane, tex * U * 8 * 2);
    }
    const size_t tw_entries = (size_t)n + 128 + ocean::stage_twiddle_entries(n);
    ok = ok && alloc((void**)&c->tw, tw_entries * 8);
    ok = ok && alloc((void**)&c->casc, 5 * 4 * 5);
    if (!ok) {
        std::string msg = std::string("device allocation failed: ") + hipGetErrorString(hipGetLastError());
        free_all(c);
        delete c;
        return fail(OCEAN_E_OUT_OF_MEMORY, msg);
    }
    // twiddle table tw[m] = exp(+2 pi i m / N), double precision then rounded
    std::vector<float2> tw(tw_entries);
    for (int m = 0; m < n; ++m) {
        const double a = 2.0 * M_PI * (double)m / (double)n;
        tw[m] = make_float2((float)std::cos(a), (float)std::sin(a));
    }
    for (int k = 0; k < 64; ++k) {
        const double lo = 2.0 * M_PI * (double)k / (double)n, hi = 2.0 * M_PI * 64.0 * (double)k / (double)n;
        tw[n + k] = make_float2((float)std::cos(lo), (float)std::sin(lo));
        tw[n + 64 + k] = make_float2((float)std::cos(hi), (float)std::sin(hi));
    }
    // per-stage tables for the plans with first radix 16, 8 and 4 (fft_engine.h StageTw):
    // stage s >= 1 (Ns, R), entry r*Ns + k = exp(+2 pi i r k / (Ns R))
    {
        using namespace ocean::fftcore;
        size_t o = (size_t)n + 128;
        for (int r0 : {16, 8, 4})
            for (int s = 1; s < n_stages(n, r0); ++s) {
                const int ns = ns_of(n, s, r0), r = radix_of(n, s, r0);
                for (int q = 0; q < r; ++q)
                    for (int k = 0; k < ns; ++k) {
                        const double a = 2.0 * M_PI * (double)q * (double)k / ((double)ns * (double)r);
                        tw[o++] = make_float2((float)std::cos(a), (float)std::sin(a));
                    }
            }
    }
    e = hipMemcpy(c->tw, tw.data(), tw_entries * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        free_all(c);
        delete c;
        return hip_fail(e, "twiddle upload");
    }
    *out = c;
    return OCEAN_OK;
}

void ocean_destroy(ocean_ctx* ctx) {
    if (!ctx) return;
    DeviceScope device_scope(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    free_all(ctx);
    delete ctx;
}

int ocean_set_params(ocean_ctx* ctx, const ocean_params* params, const ocean_cascade* cascades) {
    OCEAN_ENTER(ctx);
    if (!params || !cascades) return fail(OCEAN_E_INVALID_ARG, "null params/cascades");
    const ocean_params& p = *params;
    if (!(p.gravity > 0) || !(p.fetch > 0) || !(p.wind_speed > 0) || !std::isfinite(p.depth))
        return fail(OCEAN_E_INVALID_ARG, "gravity, fetch and wind_speed must be > 0, depth finite");
    if (p.wind_dir_x == 0.0f && p.wind_dir_y == 0.0f) return fail(OCEAN_E_INVALID_ARG, "zero wind direction");
    float h[25];
    for (int c = 0; c < ctx->C; ++c) {
        const ocean_cascade& k = cascades[c];
        if (!(k.wavelength > 0)) return fail(OCEAN_E_INVALID_ARG, "cascade wavelength must be > 0");
        h[c * 5 + 0] = k.wavelength;
        h[c * 5 + 1] = k.cutoff_low;
        h[c * 5 + 2] = k.cutoff_high;
        h[c * 5 + 3] = k.swell;
        h[c * 5 + 4] = k.fade;
    }
    // staged only: the running spectrum (h0, and the wave data the fused row pass rebuilds
    // every frame from casc + gravity) keeps its constants until ocean_init_spectrum
    std::memcpy(ctx->staged_casc, h, sizeof(float) * 5 * ctx->C);
    ctx->staged_params = {p.wind_speed, p.wind_dir_x, p.wind_dir_y, p.gravity, p.fetch, p.depth};
    ctx->params_set = true;
    return OCEAN_OK;
}

int ocean_set_noise(ocean_ctx* ctx, int tile, const float* rg) {
    OCEAN_ENTER(ctx);
    if (!rg) return fail(OCEAN_E_INVALID_ARG, "null noise");
    char* dst = nullptr;
    if (int r = slice_ptr(ctx, OCEAN_TEX_NOISE, tile, 0, ctx->texels() * 8, &dst)) return r;
    OCEAN_HIP(hipMemcpyAsync(dst, rg, ctx->texels() * 8, hipMemcpyHostToDevice, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    ctx->noise_set[tile] = true;
    return OCEAN_OK;
}

int ocean_generate_noise_device(ocean_ctx* ctx, uint64_t seed) {
    OCEAN_ENTER(ctx);
    const ocean::DevView v = ctx->view();
    OCEAN_HIP(ocean::launch_noise(v, seed, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    for (int t = 0; t < ctx->T; ++t) ctx->noise_set[t] = true;
    return OCEAN_OK;
}

int ocean_generate_noise(ocean_ctx* ctx, uint64_t seed) {
    OCEAN_ENTER(ctx);
    std::vector<float> host(ctx->texels() * 2);
    for (int t = 0; t < ctx->T; ++t) {
        ocean::generate_noise_host(ctx->n, seed + (uint64_t)t, host.data());
        if (int r = ocean_set_noise(ctx, t, host.data())) return r;
    }
    return OCEAN_OK;
}

namespace {
// Band-limited cascades: the live extent of every unit reduced from the new h0k, read back, and pass AQ's
// item table built from it (prune_items.h).  The side arrays are cleared with it, but nothing relies on that:
// they are per chunk slot and reused by every chunk of a frame, so what keeps pass BQ from the d0 and srow of
// rows no item wrote is its own live-row test (fftq.hip is_live), as for the intermediate.
int rebuild_prune(ocean_ctx* ctx) {
    ctx->prune_ready = false;
    if (!ctx->prune_dev) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    const int U = (int)ctx->units();
    OCEAN_HIP(ocean::launch_live_extent(v, ctx->prune_dev, ctx->stream));
    std::vector<int> ext((size_t)U);
    OCEAN_HIP(hipMemcpyAsync(ext.data(), ctx->prune_dev, (size_t)U * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipMemsetAsync(ctx->qside, 0, ctx->inter_units * 2 * ctx->n * 8, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    ctx->prune.build(ext.data(), U, ctx->n);
    if (!ctx->prune.items.empty())
        OCEAN_HIP(hipMemcpyAsync(ctx->prune_dev + U, ctx->prune.items.data(), ctx->prune.items.size() * sizeof(int),
                                 hipMemcpyHostToDevice, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));  // the table is pageable host memory
    ctx->prune_ready = true;
    return OCEAN_OK;
}
}  // namespace

int ocean_init_spectrum(ocean_ctx* ctx) {
    OCEAN_ENTER(ctx);
    if (!ctx->params_set) return fail(OCEAN_E_STATE, "ocean_set_params must precede ocean_init_spectrum");
    for (int t = 0; t < ctx->T; ++t)
        if (!ctx->noise_set[t]) return fail(OCEAN_E_STATE, "noise not set for tile " + std::to_string(t));
    // the staged parameters become active (stream-ordered: frames queued before this
    // call still read the previous constants)
    OCEAN_HIP(hipMemcpyAsync(ctx->casc, ctx->staged_casc, (size_t)ctx->C * 5 * 4, hipMemcpyHostToDevice, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    ctx->params = ctx->staged_params;
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2, [&] { return ocean::launch_init_spectrum(v, ctx->params, ctx->stream); },
                      "init_spectrum"))
        return r;
    if (int r = timed(ctx, 2, [&] { return ocean::launch_conjugate(v, ctx->stream); }, "conjugate")) return r;
    // the foam state is left alone: the reference re-runs CalculateInitialSpectrumTextures on a
    // parameter change (the commented OnValidate, WaterBody.cs:324-337) without touching
    // _TurbulenceTextures; it starts at zero (ocean_create) and ocean_reset_foam clears it
    ctx->spectrum_ready = true;
    ctx->h0k_valid = ctx->h0k != nullptr;
    ctx->h0_conj = true;
    return rebuild_prune(ctx);
}

int ocean_reset_foam(ocean_ctx* ctx) {
    OCEAN_ENTER(ctx);
    if (ctx->turb) OCEAN_HIP(hipMemsetAsync(ctx->turb, 0, ctx->texels() * ctx->units() * 16, ctx->stream));
    ctx->turb_stale = false;  // deferred TURB: the array and the foam state are both zero, so the array is whole
    if (ctx->foam) OCEAN_HIP(hipMemsetAsync(ctx->foam, 0, ctx->texels() * ctx->units() * 4, ctx->stream));
    if (ctx->turb_mips) OCEAN_HIP(hipMemsetAsync(ctx->turb_mips, 0, ctx->mip_chain * ctx->units() * 16, ctx->stream));
    return OCEAN_OK;
}

int ocean_read(ocean_ctx* ctx, int texture, int tile, int cascade, void* dst, size_t bytes) {
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    char* src = nullptr;
    if (int r = slice_ptr(ctx, texture, tile, cascade, bytes, &src)) return r;
    if (texture == OCEAN_TEX_TURB)  // deferred TURB: the array from the foam state first
        if (int r = materialise_turb(ctx)) return r;
    OCEAN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

namespace {
// Level `level` (>= 1) of slice (tile, cascade) of DERIV / TURB's mip chain.
int mip_slice_ptr(ocean_ctx* ctx, int texture, int tile, int cascade, int level, char** out, size_t* bytes) {
    if (!(ctx->flags & OCEAN_F_MIPS)) return fail(OCEAN_E_STATE, "context created without OCEAN_F_MIPS");
    if (texture != OCEAN_TEX_DERIV && texture != OCEAN_TEX_TURB)
        return fail(OCEAN_E_INVALID_ARG, "mip chains exist for OCEAN_TEX_DERIV and OCEAN_TEX_TURB only");
    if (level < 1 || (ctx->n >> level) < 1) return fail(OCEAN_E_INVALID_ARG, "mip level out of range");
    if (tile < 0 || tile >= ctx->T || cascade < 0 || cascade >= ctx->C)
        return fail(OCEAN_E_INVALID_ARG, "tile or cascade out of range");
    size_t off = 0;
    for (int l = 1; l < level; ++l) off += (size_t)(ctx->n >> l) * (ctx->n >> l);
    float4* chain = texture == OCEAN_TEX_DERIV ? ctx->deriv_mips : ctx->turb_mips;
    const size_t slice = (size_t)tile * ctx->C + cascade;
    *out = reinterpret_cast<char*>(chain + slice * ctx->mip_chain + off);
    *bytes = (size_t)(ctx->n >> level) * (ctx->n >> level) * 16;
    return OCEAN_OK;
}
}  // namespace

int ocean_read_mip(ocean_ctx* ctx, int texture, int tile, int cascade, int level, void* dst, size_t bytes) {
    if (level == 0) return ocean_read(ctx, texture, tile, cascade, dst, bytes);
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    char* src = nullptr;
    size_t want = 0;
    if (int r = mip_slice_ptr(ctx, texture, tile, cascade, level, &src, &want)) return r;
    if (bytes != want)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != mip slice size " +
                                             std::to_string(want));
    OCEAN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

int ocean_get_mip_ptr(ocean_ctx* ctx, int texture, int level, void** ptr, size_t* slice_stride) {
    if (!ctx || !ptr || !slice_stride) return fail(OCEAN_E_INVALID_ARG, "null argument");
    char* p = nullptr;
    size_t bytes = 0;
    if (int r = mip_slice_ptr(ctx, texture, 0, 0, level, &p, &bytes)) return r;
    *ptr = p;
    *slice_stride = ctx->mip_chain * 16;
    return OCEAN_OK;
}

int ocean_write(ocean_ctx* ctx, int texture, int tile, int cascade, const void* src, size_t bytes) {
    OCEAN_ENTER(ctx);
    if (!src) return fail(OCEAN_E_INVALID_ARG, "null source");
    if (texture == OCEAN_TEX_WAVES && !(ctx->flags & OCEAN_F_UNFUSED))
        return fail(OCEAN_E_UNSUPPORTED, "WAVES is read-only under the fused schedule (its row pass rebuilds the "
                                         "wave data from the parameters every frame); create the context with "
                                         "OCEAN_F_UNFUSED to drive ocean_step from uploaded wave data");
    char* dst = nullptr;
    if (int r = slice_ptr(ctx, texture, tile, cascade, bytes, &dst)) return r;
    if (texture == OCEAN_TEX_TURB)  // deferred TURB: the other slices are whole before the import below reads them
        if (int r = materialise_turb(ctx)) return r;
    OCEAN_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    if (texture == OCEAN_TEX_NOISE) ctx->noise_set[tile] = true;
    if (texture == OCEAN_TEX_DISP) drop_bounds(ctx);
    if (texture == OCEAN_TEX_H0) {  // the v3 row pass reads h0 (.zw included); the three-plane frame
        ctx->h0k_valid = false;     // needs .zw = conj h0(-k), which an upload need not keep
        ctx->h0_conj = false;
    }
    if (texture == OCEAN_TEX_TURB) {  // foam state follows the uploaded TURB.x (resume)
        const ocean::DevView v = ctx->view();
        OCEAN_HIP(ocean::launch_foam_import(v, ctx->stream));
        OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    }
    return OCEAN_OK;
}

int ocean_get_device_ptr(ocean_ctx* ctx, int texture, void** ptr, size_t* bytes) {
    if (!ctx || !ptr || !bytes) return fail(OCEAN_E_INVALID_ARG, "null argument");
    if (texture < OCEAN_TEX_NOISE || texture > OCEAN_TEX_VELOCITY) return fail(OCEAN_E_INVALID_ARG, "unknown texture id");
    size_t eb = 0, slices = 0;
    void* base = tex_ptr(ctx, texture, &eb, &slices);
    if (!base) return fail(OCEAN_E_INVALID_ARG, "texture not allocated for this context's flags");
    if (texture == OCEAN_TEX_DISP) ctx->disp_exposed = true;  // a foreign writer: the surface bounds are not cached
    if (texture == OCEAN_TEX_TURB) {
        // a foreign reader: the array is made whole now (stream-ordered, like the frames), and from here on every
        // frame writes it (frame_plan.h defer_turb), for the life of the context
        OCEAN_ENTER(ctx);
        if (int r = materialise_turb(ctx)) return r;
        ctx->turb_exposed = true;
    }
    *ptr = base;
    *bytes = ctx->texels() * eb * slices;
    return OCEAN_OK;
}

int ocean_get_stream(ocean_ctx* ctx, void** stream) {
    if (!ctx || !stream) return fail(OCEAN_E_INVALID_ARG, "null argument");
    *stream = (void*)ctx->stream;
    return OCEAN_OK;
}

int ocean_synchronize(ocean_ctx* ctx) {
    OCEAN_ENTER(ctx);
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

int ocean_set_column_band(ocean_ctx* ctx, int x_begin, int x_count) {
    OCEAN_ENTER(ctx);
    const int n = ctx->n;
    if ((ctx->flags & OCEAN_F_VELOCITY) && (x_begin != 0 || x_count != n))
        return fail(OCEAN_E_UNSUPPORTED, "a velocity context (OCEAN_F_VELOCITY) computes the whole band only");
    const int g = std::min(n, std::max(16, 8192 / n));  // a multiple of every tile width of the fused passes
    if (x_begin < 0 || x_count < 1 || x_begin + x_count > n || x_begin % g || x_count % g)
        return fail(OCEAN_E_INVALID_ARG, "column band [" + std::to_string(x_begin) + ", +" + std::to_string(x_count) +
                                             ") must lie in [0, N) with start and width multiples of " +
                                             std::to_string(g));
    if (x_count != n && (ctx->flags & (OCEAN_F_UNFUSED | OCEAN_F_MIPS)))
        return fail(OCEAN_E_UNSUPPORTED, "a column band needs the fused schedule and no mip chains");
    // deferred TURB: a band's frames write their own columns of TURB only, so the rest is made whole first (the
    // whole band keeps deferring: nothing to write)
    if (x_count != n)
        if (int r = materialise_turb(ctx)) return r;
    drop_bounds(ctx);
    ctx->band_x0 = x_begin;
    ctx->band_nx = x_count;
    ctx->col_par = -1;  // a band replaces a column parity
    return OCEAN_OK;
}

int ocean_set_column_parity(ocean_ctx* ctx, int parity) {
    OCEAN_ENTER(ctx);
    if ((ctx->flags & OCEAN_F_VELOCITY) && parity != -1)
        return fail(OCEAN_E_UNSUPPORTED, "a velocity context (OCEAN_F_VELOCITY) takes no column parity");
    if (parity < -1 || parity > 1) return fail(OCEAN_E_INVALID_ARG, "parity must be -1 (off), 0 or 1");
    // deferred TURB: as ocean_set_column_band (a parity is built for N = 4096, whose frames never defer, so this
    // launches nothing today)
    if (int r = materialise_turb(ctx)) return r;
    drop_bounds(ctx);
    if (parity < 0) {
        ctx->col_par = -1;
        ctx->band_x0 = 0;
        ctx->band_nx = ctx->n;
        return OCEAN_OK;
    }
    if (ctx->n != 4096) return fail(OCEAN_E_UNSUPPORTED, "a column parity is built for N = 4096 (pass A3P)");
    if (ctx->flags & (OCEAN_F_UNFUSED | OCEAN_F_MIPS | OCEAN_F_DISPLACEMENT_ONLY))
        return fail(OCEAN_E_UNSUPPORTED, "a column parity needs the fused full-output schedule and no mip chains");
    if (!ctx->opt.q) return fail(OCEAN_E_UNSUPPORTED, "a column parity needs the three-plane frame (OCEAN_Q=0 is set)");
    // pass A3PP reads h0(k) of mirror-pair rows from h0k (8 B per texel instead of h0's 16): allocated on
    // the first parity, then kept up to date by ocean_init_spectrum (k_conjugate writes it)
    if (!ctx->h0k) {
        const size_t bytes = ctx->texels() * ctx->units() * 8;
        OCEAN_HIP(hipMalloc((void**)&ctx->h0k, bytes));
        ctx->h0k_valid = false;
    }
    // extract whenever the spectrum exists (h0.zw = conj h0(-k)) and h0k does not match it yet: a failed
    // extract leaves h0k_valid false, so the next call retries it; before ocean_init_spectrum there is
    // nothing to extract, and the init fills h0k itself
    if (!ctx->h0k_valid && ctx->h0_conj) {
        const ocean::DevView v = ctx->view();
        OCEAN_HIP(ocean::launch_h0k_extract(v, ctx->stream));
        OCEAN_HIP(hipStreamSynchronize(ctx->stream));
        ctx->h0k_valid = true;
    }
    ctx->col_par = parity;
    ctx->band_x0 = 0;
    ctx->band_nx = ctx->n / 2;  // compact: column m of every texture holds x = 2 m + parity
    return OCEAN_OK;
}

}  // extern "C"
