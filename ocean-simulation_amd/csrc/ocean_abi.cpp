// C-ABI layer of liboceanhip.so: context lifetime, validation, device memory,
// the per-frame schedule, readback and kernel timing.  See include/ocean/ocean.h
// for the reference interface each entry point replaces.
#include <cxxabi.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <algorithm>
#include <map>
#include <memory>
#include <mutex>
#include <tuple>
#include <string>
#include <vector>

#include "fft_core.h"
#include "device_scope.h"
#include "frame_plan.h"
#include "ocean_internal.h"

namespace {

thread_local std::string g_last_error;

int fail(int code, const std::string& msg) {
    g_last_error = msg;
    return code;
}

int hip_fail(hipError_t e, const char* what) {
    return fail(OCEAN_E_DEVICE, std::string(what) + ": " + hipGetErrorString(e));
}

#define OCEAN_HIP(call)                                   \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return hip_fail(_e, #call); \
    } while (0)

struct TimedLaunch {
    int kind;
    hipEvent_t a, b;
};

}  // namespace

namespace ocean {
LaunchEvents*& launch_events() {
    thread_local LaunchEvents* slot = nullptr;
    return slot;
}
const void*& last_kernel() {
    thread_local const void* slot = nullptr;
    return slot;
}

namespace {
std::mutex g_occ_mu;
std::map<std::tuple<int, const void*, int>, int> g_occ;  // (device, kernel, threads) -> per CU
std::map<int, int> g_cus;                                 // device -> CUs
int current_device() {
    int dev = 0;
    (void)hipGetDevice(&dev);
    return dev;
}
}  // namespace

int resident_per_cu(const void* kernel, int threads) {
    const auto key = std::make_tuple(current_device(), kernel, threads);
    std::lock_guard<std::mutex> lk(g_occ_mu);
    auto it = g_occ.find(key);
    if (it != g_occ.end()) return it->second;
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, kernel, threads, 0) != hipSuccess || per_cu <= 0)
        per_cu = 1;
    g_occ.emplace(key, per_cu);
    return per_cu;
}

int device_cus() {
    const int dev = current_device();
    std::lock_guard<std::mutex> lk(g_occ_mu);
    auto it = g_cus.find(dev);
    if (it != g_cus.end()) return it->second;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) cus = 256;
    g_cus.emplace(dev, cus);
    return cus;
}
}  // namespace ocean

// Host noise generator (WaterBody.cs:71-100 with this library's documented
// uniform source).  Defined in noise.cpp.
namespace ocean {
void generate_noise_host(int n, uint64_t seed, float* out);
}

// Staging slots of the readback requests (every *_async entry).  A slot is device memory as large as one
// slice of the largest texture plus the events of the request holding it, created once with the slot: no
// event is created per request.  `after` and `done` disable timing; the timed pair `tstart` / `tdone`
// (ocean_readback_copy_ms) is created on the slot's first request made with readback timing on
// (ocean_set_readback_timing) and recorded only for such requests.  A request takes a slot and gives it back
// when it is released (after its host copy has landed), so a slot is never rewritten while a copy out of
// it is pending, and no allocation or free sits between the context stream and the copy stream.  Shared
// with the requests: it outlives a context destroyed before its requests are released.
// A request that runs a kernel over inputs of the caller's (start_staged_readback) lays the slot out in one
// way: the kernel's results at the base, which is what the host copy reads; the inputs, back to back, from
// kQueryPointsOffset on; and, from the slot's first such request on, a pinned host copy of the inputs
// (`pts_host`), so that the caller's buffers are consumed inside the call and the upload reads memory that
// stays put until the request is released.  Sized by the largest point query; the other consumers assert
// that they fit.  One consumer's inputs outgrow the 512 KiB behind kQueryPointsOffset: ocean_body_dynamics_async
// stages 592 KiB at its limits, so its inputs start at kDynamicsInputOffset, right behind its own smaller
// results (the arithmetic is at the entry), and the pinned copy is sized for it (kStageInputBytes).
constexpr size_t kQueryPointsOffset = (size_t)OCEAN_QUERY_MAX_POINTS * 8 * sizeof(float);
constexpr size_t kQuerySlotBytes = kQueryPointsOffset + (size_t)OCEAN_QUERY_MAX_POINTS * 2 * sizeof(float);
constexpr size_t kDynamicsInputOffset = (size_t)OCEAN_BODY_MAX_BODIES * 16 * sizeof(float);
constexpr size_t kDynamicsInputBytes = (size_t)OCEAN_BODY_MAX_BODIES * (10 + 6) * sizeof(float) +
                                       (size_t)OCEAN_BODY_MAX_PROBES * 5 * sizeof(float);
constexpr size_t kStageInputBytes = std::max(kQuerySlotBytes - kQueryPointsOffset, kDynamicsInputBytes);
// Workgroup tile of the grid kernel (grid.hip), nodes along x: the fastest of the shapes measured.
constexpr int kGridTileDefault = 32;
struct StageSlot {
    void* mem = nullptr;
    void* pts_host = nullptr;    // pinned, kStageInputBytes: the inputs of the request holding the slot
    hipEvent_t after = nullptr;  // the snapshot is in the slot (the copy stream waits for it)
    hipEvent_t done = nullptr;   // the host copy has landed (untimed requests)
    hipEvent_t tstart = nullptr, tdone = nullptr;  // timed requests: around the host copy itself
};
struct StagePool {
    int device = 0;
    size_t slot_bytes = 0;
    std::mutex mu;
    std::vector<StageSlot*> free_slots, all;
    ~StagePool() {
        int prev = 0;
        const bool had = hipGetDevice(&prev) == hipSuccess;
        (void)hipSetDevice(device);
        for (StageSlot* sl : all) {
            if (sl->mem) (void)hipFree(sl->mem);
            if (sl->pts_host) (void)hipHostFree(sl->pts_host);
            for (hipEvent_t e : {sl->after, sl->done, sl->tstart, sl->tdone})
                if (e) (void)hipEventDestroy(e);
            delete sl;
        }
        if (had) (void)hipSetDevice(prev);  // the caller's current device is left as it was
    }
    hipError_t take(bool timed, StageSlot** out) {
        std::lock_guard<std::mutex> lk(mu);
        if (free_slots.empty()) {
            StageSlot* sl = new (std::nothrow) StageSlot();
            if (!sl) return hipErrorOutOfMemory;
            hipError_t e = hipMalloc(&sl->mem, slot_bytes);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sl->after, hipEventDisableTiming);
            if (e == hipSuccess) e = hipEventCreateWithFlags(&sl->done, hipEventDisableTiming);
            all.push_back(sl);  // freed with the pool even when incomplete
            if (e != hipSuccess) return e;
            free_slots.push_back(sl);
        }
        StageSlot* sl = free_slots.back();
        if (timed && !sl->tstart) {  // both timed events, or neither
            hipEvent_t a = nullptr, b = nullptr;
            hipError_t e = hipEventCreate(&a);
            if (e == hipSuccess) e = hipEventCreate(&b);
            if (e != hipSuccess) {
                if (a) (void)hipEventDestroy(a);
                return e;
            }
            sl->tstart = a;
            sl->tdone = b;
        }
        free_slots.pop_back();
        *out = sl;
        return hipSuccess;
    }
    void give(StageSlot* sl) {
        std::lock_guard<std::mutex> lk(mu);
        free_slots.push_back(sl);
    }
};

// Environment knobs of a context, read once in ocean_create ("Environment knobs";
// tests/test_abi.py checks that this is every getenv of the library).  The defaults are the measured
// best; every knob changes the schedule only, never the arithmetic of a texel, except OCEAN_Q and
// OCEAN_A4, which select the reference's four-plane passes (within the fp32 tolerance / bit-identical).
struct ocean_options {
    int q = 1;              // OCEAN_Q=0: the four-plane fused frame where the three-plane one applies
    int a4 = 1;             // OCEAN_A4=0: the per-texel row pass A3 instead of the mirror-pair pass A4
    long chunk_mib = 192;   // OCEAN_CHUNK_MIB: intermediate MiB per unit chunk of a frame (0: whole frame)
    int c4_bands = 0;       // OCEAN_C4_BANDS: N >= 2048 column passes per (unit, band); 0 = auto
    long op_chunk_mib = 0;  // OCEAN_OP_CHUNK_MIB: MiB of unit-planes per chunk of ocean_ifft2d (0: auto)
    int tile_w = 0;         // OCEAN_TILE_W: column-tile width of the fused path at N = 128..1024 (0: auto)
    int disp_cached = -1;   // OCEAN_DISP_CACHED: 0 / 1 force pass BQ's DISP store policy (disp_fits_cache); -1 auto
    int grid_tile = 0;      // OCEAN_GRID_TILE: nodes along x of the grid kernel's workgroup tile, 64 / 32 / 16 (0: kept)
    int vel_nt = 0;         // OCEAN_VEL_NT=1: the velocity pack kernel writes VEL with nontemporal stores
    int prune = 1;          // OCEAN_PRUNE=0: passes AQ / BQ run every row of a band-limited cascade (dense schedule)
    int ray_bounds = 1;     // OCEAN_RAY_BOUNDS=0: the ray kernel samples every node (no air skip, no bounds launches)
    int max_groups = 0;     // OCEAN_MAX_GROUPS: at most this many workgroups per persistent launch (the transform passes
                            // of fftq / fft3 / fft4k / fft2.hip), so that their item loops iterate at small shapes; 0: no cap

    static ocean_options from_env() {
        ocean_options o;
        if (const char* e = std::getenv("OCEAN_Q")) o.q = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_A4")) o.a4 = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_CHUNK_MIB")) o.chunk_mib = std::max(0L, std::atol(e));
        if (const char* e = std::getenv("OCEAN_C4_BANDS")) o.c4_bands = std::max(0, std::atoi(e));
        if (const char* e = std::getenv("OCEAN_OP_CHUNK_MIB")) o.op_chunk_mib = std::max(0L, std::atol(e));
        if (const char* e = std::getenv("OCEAN_TILE_W")) o.tile_w = std::max(0, std::atoi(e));
        if (const char* e = std::getenv("OCEAN_DISP_CACHED")) o.disp_cached = std::strcmp(e, "auto") ? std::atoi(e) != 0 : -1;
        if (const char* e = std::getenv("OCEAN_GRID_TILE")) o.grid_tile = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_VEL_NT")) o.vel_nt = std::atoi(e) != 0;
        if (const char* e = std::getenv("OCEAN_PRUNE")) o.prune = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_RAY_BOUNDS")) o.ray_bounds = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_MAX_GROUPS")) o.max_groups = std::max(0, std::atoi(e));
        return o;
    }
};

struct ocean_ctx {
    int device = 0;
    int n = 0, logn = 0, C = 0, T = 0, P = 4;
    uint32_t flags = 0;
    hipStream_t stream = nullptr;
    // device buffers
    float2* noise = nullptr;
    float4* h0 = nullptr;
    float2* h0k = nullptr;   // h0.xy for the mirror-pair row passes: pass_a4_supported sizes, and pass A3PP
                             // at N = 4096 (allocated by ocean_set_column_parity)
    bool h0k_valid = false;  // h0k matches h0 (false after ocean_write(H0): .zw may then be arbitrary)
    bool h0_conj = false;    // h0.zw = conj h0(-k) (from ocean_init_spectrum; the three-plane frame needs it)
    ocean_options opt;       // environment knobs, read once in ocean_create
    size_t inter_units = 0;  // units the intermediate holds (one chunk of a frame; every chunk reuses it)
    int band_x0 = 0, band_nx = 0;  // column band of the fused passes (ocean_set_column_band); nx = n: whole
    int col_par = -1;              // column parity (ocean_set_column_parity): -1 off, else x = 2 m + col_par
    int tile_w = 8;                // column-tile width of the fused path's tile-major layouts (ocean_create)
    float4* waves = nullptr;
    float2* plane[4] = {nullptr, nullptr, nullptr, nullptr};
    float4* disp = nullptr;
    float4* deriv = nullptr;
    float4* turb = nullptr;
    float4* normal = nullptr;
    float4* vel = nullptr;     // OCEAN_F_VELOCITY: the VELOCITY texture ...
    float2* vplane = nullptr;  // ... and its two scratch planes, [2][U][N][N] plane-major (velocity.hip)
    float2* tw = nullptr;
    float* casc = nullptr;
    float2* tplane = nullptr;  // fused-path intermediate (tile-major), P planes
    float* foam = nullptr;     // foam state (tile-major)
    float2* qside = nullptr;   // three-plane frame side arrays (d0, srow per unit of a chunk)
    // band-limited cascades (fftq.hip PRUNE): per-unit live extents [U], then pass AQ's item table, on the
    // device; their host copy; valid from ocean_init_spectrum on (the frame uses them only while use_q holds,
    // that is while h0k is the spectrum they were reduced from)
    int* prune_dev = nullptr;
    ocean::PruneItems prune;
    bool prune_ready = false;
    // surface bounds (bounds.hip), allocated by the first entry that needs them: the records float[T][C][8],
    // then pass 1's partials.  bounds_valid[t]: tile t's records match DISP (dropped by every entry that writes
    // DISP).  disp_exposed: ocean_get_device_ptr has handed DISP out, a foreign writer cannot be seen, so
    // nothing is cached any more and every use recomputes.
    float* bounds_dev = nullptr;
    std::vector<bool> bounds_valid;
    bool disp_exposed = false;
    // whitecap emitters (whitecaps.hip): the ballot masks and per-chunk counts of the largest grid, allocated by the
    // first ocean_whitecaps* call and reused by every later one
    void* whitecap_dev = nullptr;
    float4* deriv_mips = nullptr;  // OCEAN_F_MIPS chains (levels 1..log2 N per slice)
    float4* turb_mips = nullptr;
    size_t mip_chain = 0;
    hipStream_t copy_stream = nullptr;  // the host copies of the readback requests (every *_async entry)
    std::shared_ptr<StagePool> stage_pool;  // their staging slots
    bool readback_timing = false;           // ocean_set_readback_timing
    // host state.  `params` and the device `casc` are what the kernels run with; set_params
    // only stages new values, which ocean_init_spectrum makes active (ocean.h), so a
    // frame stepped between the two still uses the spectrum's own constants.
    ocean::SpectrumParams params{};
    ocean::SpectrumParams staged_params{};
    float staged_casc[5 * ocean::kMaxCascades] = {};
    bool params_set = false;
    std::vector<bool> noise_set;
    bool spectrum_ready = false;
    // timing
    bool timing = false;
    std::vector<hipEvent_t> event_pool;
    std::vector<TimedLaunch> pending;
    double kind_ms[3] = {0, 0, 0};
    long long kind_count[3] = {0, 0, 0};
    const void* kind_kernel[3] = {nullptr, nullptr, nullptr};  // last kernel launched per kind (ocean_kernel_name)
    static constexpr size_t kMaxPending = 2048;  // timed launches held before folding into kind_ms

    size_t texels() const { return (size_t)n * n; }
    size_t units() const { return (size_t)T * C; }

    // what the frame schedule reads of a context (frame_plan.h)
    ocean::FrameInputs frame_inputs() const {
        return {{n, C, T, P, inter_units, band_x0, band_nx, col_par},
                {opt.q, opt.a4, opt.chunk_mib, opt.c4_bands, opt.disp_cached},
                {h0k != nullptr, qside != nullptr, h0k_valid, h0_conj, prune_ready, &prune}};
    }

    ocean::DevView view() const {
        ocean::DevView v{};
        v.n = n;
        v.logn = logn;
        v.C = C;
        v.T = T;
        v.units = T * C;
        v.planes = P;
        v.normals = (flags & OCEAN_F_NORMALS) != 0;
        v.max_groups = opt.max_groups;
        v.noise = noise;
        v.h0 = h0;
        v.h0k = h0k;
        v.waves = waves;
        for (int p = 0; p < 4; ++p) v.plane[p] = plane[p];
        v.plane_stride = texels() * units();
        v.inter_stride = texels() * inter_units;
        v.disp = disp;
        v.deriv = deriv;
        v.turb = turb;
        v.normal = normal;
        v.tw = tw;
        v.casc = casc;
        v.gravity = params.gravity;
        v.tile_w = tile_w;
        v.tplane = tplane;
        v.foam = foam;
        v.qside = qside;
        v.deriv_mips = deriv_mips;
        v.turb_mips = turb_mips;
        v.mip_chain = mip_chain;
        v.x0 = band_x0;
        v.nx = band_nx;
        v.xstr = col_par >= 0 ? 2 : 1;
        v.xpar = col_par >= 0 ? col_par : 0;
        return v;
    }

    hipEvent_t take_event() {
        if (event_pool.empty()) {
            hipEvent_t e = nullptr;
            if (hipEventCreate(&e) != hipSuccess) return nullptr;
            return e;
        }
        hipEvent_t e = event_pool.back();
        event_pool.pop_back();
        return e;
    }
};

namespace {

// The device rule of every entry point (device_scope.h) over the HIP runtime: hipSetDevice only when the
// device differs, and a failure to set it becomes the call's OCEAN_E_DEVICE.
struct HipDeviceApi {
    static int get(int* device) { return (int)hipGetDevice(device); }
    static int set(int device) { return (int)hipSetDevice(device); }
};
class DeviceScope : public ocean::BasicDeviceScope<HipDeviceApi> {
  public:
    explicit DeviceScope(int device) : ocean::BasicDeviceScope<HipDeviceApi>(device) {
        if (error()) status_ = hip_fail((hipError_t)error(), "hipSetDevice");
    }
    int status() const { return status_; }

  private:
    int status_ = OCEAN_OK;
};

}  // namespace

// Entry of every call that touches the device: check the context, make its device current until the
// call returns (DeviceScope), or return the failure.
#define OCEAN_ENTER(ctx)                                                        \
    if (!(ctx)) return fail(OCEAN_E_INVALID_ARG, "null context");              \
    DeviceScope device_scope_((ctx)->device);                                   \
    if (const int device_scope_status_ = device_scope_.status()) return device_scope_status_

namespace {

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

// Launch wrapper: when kernel timing is on, the kernels launched by `launch` carry an event
// pair (ocean_internal.h, launch_events).  A host that never polls ocean_kernel_stats holds
// at most kMaxPending launches' events.
template <class F>
int timed(ocean_ctx* ctx, int kind, F&& launch, const char* what) {
    ocean::last_kernel() = nullptr;
    if (!ctx->timing) {
        const hipError_t e = launch();
        if (ocean::last_kernel()) ctx->kind_kernel[kind] = ocean::last_kernel();
        return e == hipSuccess ? OCEAN_OK : hip_fail(e, what);
    }
    if (ctx->pending.size() >= ocean_ctx::kMaxPending) {
        if (int r = fold_pending(ctx, false)) return r;
        if (ctx->pending.size() >= ocean_ctx::kMaxPending)
            if (int r = fold_pending(ctx, true)) return r;
    }
    ocean::LaunchEvents ev{ctx->take_event(), ctx->take_event(), false};
    if (!ev.start || !ev.stop) return fail(OCEAN_E_DEVICE, "hipEventCreate failed");
    ocean::launch_events() = &ev;  // the kernels of this entry carry the events (ocean_internal.h)
    const hipError_t e = launch();
    ocean::launch_events() = nullptr;
    if (ocean::last_kernel()) ctx->kind_kernel[kind] = ocean::last_kernel();
    if (e != hipSuccess) return hip_fail(e, what);
    if (!ev.launched) {  // nothing was launched: an empty interval
        OCEAN_HIP(hipEventRecord(ev.start, ctx->stream));
        OCEAN_HIP(hipEventRecord(ev.stop, ctx->stream));
    }
    ctx->pending.push_back({kind, ev.start, ev.stop});
    return OCEAN_OK;
}

// Every entry that writes DISP drops the cached surface bounds (ocean.h ocean_surface_bounds).
void drop_bounds(ocean_ctx* ctx) { ctx->bounds_valid.assign(ctx->bounds_valid.size(), false); }

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

void free_all(ocean_ctx* c) {
    void* ptrs[] = {c->noise, c->h0, c->h0k, c->waves, c->plane[0], c->disp, c->deriv,
                    c->turb,  c->normal, c->tw,    c->casc,     c->tplane, c->foam, c->deriv_mips, c->turb_mips,
                    c->qside, c->vel, c->vplane, c->prune_dev, c->bounds_dev, c->whitecap_dev};
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
    if (ctx->foam) OCEAN_HIP(hipMemsetAsync(ctx->foam, 0, ctx->texels() * ctx->units() * 4, ctx->stream));
    if (ctx->turb_mips) OCEAN_HIP(hipMemsetAsync(ctx->turb_mips, 0, ctx->mip_chain * ctx->units() * 16, ctx->stream));
    return OCEAN_OK;
}

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
    return timed(ctx, 2, [&] { return ocean::launch_fill(v, ctx->stream); }, "fill");
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
    return ocean::plan_frame(in, [&](const ocean::FrameStep& st) {
        ocean::DevView c = sub_view(v, st.u0, st.nu, st.inter_u0);
        c.x0 = st.x0;
        c.nx = st.nx;
        c.disp_cached = st.disp_cached;
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

int ocean_read(ocean_ctx* ctx, int texture, int tile, int cascade, void* dst, size_t bytes) {
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    char* src = nullptr;
    if (int r = slice_ptr(ctx, texture, tile, cascade, bytes, &src)) return r;
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

}  // extern "C"

struct ocean_readback {
    int device = 0;
    bool timed = false;  // made with readback timing on: tstart / tdone recorded
    StageSlot* slot = nullptr;
    std::shared_ptr<StagePool> pool;
    hipEvent_t done() const { return timed ? slot->tdone : slot->done; }
};

namespace {
// The host copy of the readbacks: hipMemcpyDeviceToHost (see docs/MEASUREMENTS.md section 8 for the
// engine the runtime picks)
constexpr hipMemcpyKind kReadbackCopyKind = hipMemcpyDeviceToHost;

// A readback request: `snapshot` enqueues the copy of the wanted bytes into the slot on the ctx stream
// (ordered after the queued steps and before later ones, at HBM speed), then the host copy runs on the
// copy stream, off the ctx stream's path -- snapshot semantics, like a readback in Unity's command stream.
template <class Snapshot>
int start_readback(ocean_ctx* ctx, void* dst, size_t bytes, Snapshot&& snapshot, ocean_readback** out) {
    if (!ctx->copy_stream) OCEAN_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->stage_pool) {
        ctx->stage_pool = std::make_shared<StagePool>();
        ctx->stage_pool->device = ctx->device;
        // the largest slice (float4 textures), or a full surface query's points and results (N <= 256)
        ctx->stage_pool->slot_bytes = std::max(ctx->texels() * 16, kQuerySlotBytes);
    }
    ocean_readback* rb = new (std::nothrow) ocean_readback();
    if (!rb) return fail(OCEAN_E_OUT_OF_MEMORY, "host allocation failed");
    rb->device = ctx->device;
    rb->pool = ctx->stage_pool;
    rb->timed = ctx->readback_timing;
    hipError_t e = rb->pool->take(rb->timed, &rb->slot);
    if (e == hipSuccess) e = snapshot(rb->slot);
    if (e == hipSuccess) e = hipEventRecord(rb->slot->after, ctx->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, rb->slot->after, 0);
    if (e == hipSuccess && rb->timed) e = hipEventRecord(rb->slot->tstart, ctx->copy_stream);
    if (e == hipSuccess) e = hipMemcpyAsync(dst, rb->slot->mem, bytes, kReadbackCopyKind, ctx->copy_stream);
    if (e == hipSuccess) e = hipEventRecord(rb->done(), ctx->copy_stream);
    if (e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (rb->slot) rb->pool->give(rb->slot);
        delete rb;
        return hip_fail(e, "readback request");
    }
    *out = rb;
    return OCEAN_OK;
}

// The three forms of a point consumer (world sampling, the surface and velocity queries, the surface grids,
// the buoyant bodies) share what follows; each entry keeps its own checks and its own kernel launch, a
// callable (const float* d_in, float* d_out) over device pointers that returns an OCEAN_* code.

// One array of the caller's that a host or async form stages for its kernel.  The arrays of a request lie
// back to back in the order given, the first at d_in (floats all: every offset is 4-byte aligned).
struct HostInput {
    const void* ptr;
    size_t bytes;
};

// The blocking host form: one stream-ordered block holds the inputs from its base and the output at the next
// 256-byte boundary (float4 output rows stay 16-B aligned); upload, launch, download, free, synchronize.  The
// launch's own code comes first, then the copies', the free's and the synchronize's.
template <class Launch>
int run_staged(ocean_ctx* ctx, const char* entry, std::initializer_list<HostInput> inputs, void* out,
               size_t out_bytes, Launch&& launch) {
    size_t in_bytes = 0;
    for (const HostInput& in : inputs) in_bytes += in.bytes;
    const size_t out_off = (in_bytes + 255) & ~(size_t)255;
    void* d = nullptr;
    OCEAN_HIP(hipMallocAsync(&d, out_off + out_bytes, ctx->stream));
    char* d_in = static_cast<char*>(d);
    float* d_out = reinterpret_cast<float*>(d_in + out_off);
    hipError_t e = hipSuccess;
    size_t off = 0;
    for (const HostInput& in : inputs) {
        if (e == hipSuccess) e = hipMemcpyAsync(d_in + off, in.ptr, in.bytes, hipMemcpyHostToDevice, ctx->stream);
        off += in.bytes;
    }
    int r = OCEAN_OK;
    if (e == hipSuccess) r = launch(reinterpret_cast<const float*>(d_in), d_out);
    if (e == hipSuccess && r == OCEAN_OK) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t ef = hipFreeAsync(d, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (r != OCEAN_OK) return r;
    if (e != hipSuccess) return hip_fail(e, (std::string(entry) + " copy").c_str());
    if (ef != hipSuccess) return hip_fail(ef, "hipFreeAsync");
    if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize");
    return OCEAN_OK;
}

// The async form, a readback request whose snapshot is the kernel's result (StageSlot has the layout): the
// caller's inputs are consumed here, into the pinned memory the slot owns, so the one upload that carries
// them all is truly asynchronous and reads nothing of the caller's after this call returns; the kernel
// then writes its results at the slot's base.  (start_readback reports a hipError_t, hence the bridge.)
// in_offset: where the inputs start in the slot (behind the results; the caller asserts that both fit).
template <class Launch>
int start_staged_readback(ocean_ctx* ctx, std::initializer_list<HostInput> inputs, void* dst, size_t out_bytes,
                          Launch&& launch, ocean_readback** req, size_t in_offset = kQueryPointsOffset) {
    return start_readback(
        ctx, dst, out_bytes,
        [&](StageSlot* sl) {
            char* d_in = static_cast<char*>(sl->mem) + in_offset;
            if (inputs.size() != 0) {
                if (!sl->pts_host) {
                    const hipError_t e = hipHostMalloc(&sl->pts_host, kStageInputBytes, hipHostMallocDefault);
                    if (e != hipSuccess) return e;
                }
                size_t in_bytes = 0;
                for (const HostInput& in : inputs) {
                    std::memcpy(static_cast<char*>(sl->pts_host) + in_bytes, in.ptr, in.bytes);
                    in_bytes += in.bytes;
                }
                const hipError_t e = hipMemcpyAsync(d_in, sl->pts_host, in_bytes, hipMemcpyHostToDevice, ctx->stream);
                if (e != hipSuccess) return e;
            }
            return launch(reinterpret_cast<const float*>(d_in), static_cast<float*>(sl->mem)) == OCEAN_OK
                       ? hipSuccess
                       : hipErrorLaunchFailure;
        },
        req);
}

// The _device forms: the kernels read floats and write float4 rows (ocean.h).  `inputs` names the float
// arrays `in` in the message; an entry without any passes nullptr.
int check_aligned(const char* entry, const char* inputs, std::initializer_list<const void*> in, const void* out) {
    bool ok = ((uintptr_t)out & 15) == 0;
    for (const void* p : in) ok = ok && ((uintptr_t)p & 3) == 0;
    if (ok) return OCEAN_OK;
    return fail(OCEAN_E_INVALID_ARG, std::string(entry) + ": " +
                                         (inputs ? std::string(inputs) + " must be 4-byte and out" : "out must be") +
                                         " 16-byte aligned");
}
}  // namespace

extern "C" {

int ocean_read_async(ocean_ctx* ctx, int texture, int tile, int cascade, void* dst, size_t bytes,
                     ocean_readback** out) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "out is null");
    *out = nullptr;
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    char* src = nullptr;
    if (int r = slice_ptr(ctx, texture, tile, cascade, bytes, &src)) return r;
    return start_readback(
        ctx, dst, bytes,
        [&](StageSlot* sl) { return hipMemcpyAsync(sl->mem, src, bytes, hipMemcpyDeviceToDevice, ctx->stream); },
        out);
}

int ocean_read_height_async(ocean_ctx* ctx, int tile, int cascade, float* dst, size_t bytes, ocean_readback** out) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "out is null");
    *out = nullptr;
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    if (bytes != ctx->texels() * 4)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != N * N * 4 = " +
                                             std::to_string(ctx->texels() * 4));
    char* src = nullptr;
    if (int r = slice_ptr(ctx, OCEAN_TEX_DISP, tile, cascade, ctx->texels() * 16, &src)) return r;
    return start_readback(
        ctx, dst, bytes,
        [&](StageSlot* sl) {
            return ocean::launch_extract_height(reinterpret_cast<const float4*>(src), static_cast<float*>(sl->mem),
                                                ctx->texels(), ctx->stream);
        },
        out);
}

int ocean_set_readback_timing(ocean_ctx* ctx, int enable) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    ctx->readback_timing = enable != 0;
    return OCEAN_OK;
}

int ocean_readback_status(ocean_readback* rb) {
    if (!rb) return fail(OCEAN_E_INVALID_ARG, "null readback");
    const hipError_t e = hipEventQuery(rb->done());
    if (e == hipSuccess) return 1;
    if (e == hipErrorNotReady) return 0;
    return hip_fail(e, "hipEventQuery");
}

int ocean_readback_wait(ocean_readback* rb) {
    if (!rb) return fail(OCEAN_E_INVALID_ARG, "null readback");
    OCEAN_HIP(hipEventSynchronize(rb->done()));
    return OCEAN_OK;
}

void ocean_readback_release(ocean_readback* rb) {
    if (!rb) return;
    {
        DeviceScope device_scope(rb->device);
        (void)hipEventSynchronize(rb->done());  // the slot is free only once its host copy has landed
        rb->pool->give(rb->slot);
    }
    delete rb;
}

int ocean_readback_copy_ms(ocean_readback* rb, float* ms) {
    if (!rb || !ms) return fail(OCEAN_E_INVALID_ARG, "null readback or output");
    if (!rb->timed) return fail(OCEAN_E_STATE, "request made without readback timing (ocean_set_readback_timing)");
    const hipError_t q = hipEventQuery(rb->done());
    if (q == hipErrorNotReady) return fail(OCEAN_E_STATE, "readback still pending");
    if (q != hipSuccess) return hip_fail(q, "hipEventQuery");
    OCEAN_HIP(hipEventElapsedTime(ms, rb->slot->tstart, rb->done()));
    return OCEAN_OK;
}

int ocean_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return fail(OCEAN_E_INVALID_ARG, "null out or zero size");
    *out = nullptr;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return hip_fail(e, "hipHostMalloc");
    return OCEAN_OK;
}

void ocean_host_free(void* p) {
    if (p) (void)hipHostFree(p);
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

// (the caller has entered: OCEAN_ENTER)
static int check_sample(ocean_ctx* ctx, int tile, const float* pts, int count, float* out) {
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative point count");
    if (count > 0 && (!pts || !out)) return fail(OCEAN_E_INVALID_ARG, "null points or output");
    // the cascade constants (wavelengths) the sampler divides by exist only after init
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_sample_world");
    return OCEAN_OK;
}

int ocean_sample_world_device(ocean_ctx* ctx, int tile, const float* points, int count, float* out) {
    OCEAN_ENTER(ctx);
    if (int r = check_sample(ctx, tile, points, count, out)) return r;
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "world sampling of a column-parity shard (half the columns)");
    if (int r = check_aligned("ocean_sample_world_device", "points", {points}, out)) return r;
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2, [&] { return ocean::launch_sample_world(v, tile, points, count, out, ctx->stream); },
                 "sample_world");
}

int ocean_sample_world(ocean_ctx* ctx, int tile, const float* points, int count, float* out) {
    OCEAN_ENTER(ctx);
    if (int r = check_sample(ctx, tile, points, count, out)) return r;
    if (count == 0) return OCEAN_OK;
    return run_staged(ctx, "ocean_sample_world", {{points, (size_t)count * 3 * 4}}, out, (size_t)count * 12 * 4,
                      [&](const float* d_pts, float* d_out) {
                          return ocean_sample_world_device(ctx, tile, d_pts, count, d_out);
                      });
}

// Argument checks of the surface queries, before any device call (ocean.h); `limit`: the forms that
// stage the points (host and async) take at most OCEAN_QUERY_MAX_POINTS.
static int check_query(ocean_ctx* ctx, int tile, int mode, int iterations, const float* pts, int count, float* out,
                       bool limit) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!pts || !out) return fail(OCEAN_E_INVALID_ARG, "null points or output");
    if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative point count");
    if (limit && count > OCEAN_QUERY_MAX_POINTS)
        return fail(OCEAN_E_INVALID_ARG, "point count " + std::to_string(count) + " > OCEAN_QUERY_MAX_POINTS");
    if (mode != OCEAN_QUERY_REFERENCE && mode != OCEAN_QUERY_SURFACE) return fail(OCEAN_E_INVALID_ARG, "unknown query mode");
    if (iterations < 0 || iterations > 16) return fail(OCEAN_E_INVALID_ARG, "iterations must be in [0, 16]");
    if (mode == OCEAN_QUERY_REFERENCE && iterations != 0)
        return fail(OCEAN_E_INVALID_ARG, "OCEAN_QUERY_REFERENCE takes iterations = 0");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    return OCEAN_OK;
}

// ... and of the context's state, as world sampling: the cascade wavelengths exist only after init, and a
// column-parity shard holds half the columns.
static int check_query_state(const ocean_ctx* ctx) {
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_query_surface");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "surface query of a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The query kernel on the ctx stream (device pointers; kind 2 of ocean_kernel_stats).
static int launch_query(ocean_ctx* ctx, int tile, int mode, int iterations, const float* d_pts, int count,
                        float* d_out) {
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] { return ocean::launch_query_surface(v, tile, mode, iterations, d_pts, count, d_out, ctx->stream); },
                 "query_surface");
}

int ocean_query_surface_device(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                               float* out) {
    if (int r = check_query(ctx, tile, mode, iterations, points, count, out, false)) return r;
    if (int r = check_aligned("ocean_query_surface_device", "points", {points}, out)) return r;
    if (int r = check_query_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return launch_query(ctx, tile, mode, iterations, points, count, out);
}

int ocean_query_surface(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                        float* out) {
    if (int r = check_query(ctx, tile, mode, iterations, points, count, out, true)) return r;
    if (int r = check_query_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return run_staged(ctx, "ocean_query_surface", {{points, (size_t)count * 2 * 4}}, out, (size_t)count * 8 * 4,
                      [&](const float* d_pts, float* d_out) {
                          return launch_query(ctx, tile, mode, iterations, d_pts, count, d_out);
                      });
}

int ocean_query_surface_async(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                              float* dst, ocean_readback** out) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "out is null");
    *out = nullptr;
    if (int r = check_query(ctx, tile, mode, iterations, points, count, dst, true)) return r;
    if (count == 0) return fail(OCEAN_E_INVALID_ARG, "ocean_query_surface_async: no points, so no request");
    if (int r = check_query_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {{points, (size_t)count * 2 * 4}}, dst, (size_t)count * 8 * 4,
        [&](const float* d_pts, float* d_out) { return launch_query(ctx, tile, mode, iterations, d_pts, count, d_out); },
        out);
}

// The surface-velocity queries (ocean.h): the surface query's checks (surface mode), then the context's flag
// and state.
static int check_velocity_state(const ocean_ctx* ctx) {
    if (!(ctx->flags & OCEAN_F_VELOCITY))
        return fail(OCEAN_E_UNSUPPORTED, "ocean_query_velocity needs a context created with OCEAN_F_VELOCITY");
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_query_velocity");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "velocity query of a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The velocity query kernel on the ctx stream (device pointers; kind 2 of ocean_kernel_stats).
static int launch_velocity_query(ocean_ctx* ctx, int tile, int iterations, const float* d_pts, int count, float* d_out) {
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] { return ocean::launch_query_velocity(v, ctx->vel, tile, iterations, d_pts, count, d_out, ctx->stream); },
                 "query_velocity");
}

int ocean_query_velocity_device(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* out) {
    if (int r = check_query(ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, out, false)) return r;
    if (int r = check_aligned("ocean_query_velocity_device", "points", {points}, out)) return r;
    if (int r = check_velocity_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return launch_velocity_query(ctx, tile, iterations, points, count, out);
}

int ocean_query_velocity(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* out) {
    if (int r = check_query(ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, out, true)) return r;
    if (int r = check_velocity_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return run_staged(ctx, "ocean_query_velocity", {{points, (size_t)count * 2 * 4}}, out, (size_t)count * 8 * 4,
                      [&](const float* d_pts, float* d_out) {
                          return launch_velocity_query(ctx, tile, iterations, d_pts, count, d_out);
                      });
}

int ocean_query_velocity_async(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* dst,
                               ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_query(ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, dst, true)) return r;
    if (count == 0) return fail(OCEAN_E_INVALID_ARG, "ocean_query_velocity_async: no points, so no request");
    if (int r = check_velocity_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {{points, (size_t)count * 2 * 4}}, dst, (size_t)count * 8 * 4,
        [&](const float* d_pts, float* d_out) { return launch_velocity_query(ctx, tile, iterations, d_pts, count, d_out); },
        req);
}

// Argument checks of the surface grids, before any device call (ocean.h).
static int check_grid(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx,
                      float dz, int nx, int ny, const float* out, size_t bytes) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    if (mode != OCEAN_GRID_VERTICES && mode != OCEAN_GRID_SURFACE && mode != OCEAN_GRID_HEIGHTFIELD)
        return fail(OCEAN_E_INVALID_ARG, "unknown grid mode");
    if (iterations < 0 || iterations > 16) return fail(OCEAN_E_INVALID_ARG, "iterations must be in [0, 16]");
    if (mode == OCEAN_GRID_VERTICES && iterations != 0)
        return fail(OCEAN_E_INVALID_ARG, "OCEAN_GRID_VERTICES takes iterations = 0");
    if (!std::isfinite(lod) || lod < 0.0f) return fail(OCEAN_E_INVALID_ARG, "lod must be finite and >= 0");
    if (mode != OCEAN_GRID_VERTICES && lod != 0.0f)
        return fail(OCEAN_E_INVALID_ARG, "OCEAN_GRID_SURFACE and OCEAN_GRID_HEIGHTFIELD take lod = 0");
    if (!std::isfinite(x0) || !std::isfinite(z0) || !std::isfinite(dx) || !std::isfinite(dz))
        return fail(OCEAN_E_INVALID_ARG, "grid origin and spacing must be finite");
    if (nx < 1 || ny < 1) return fail(OCEAN_E_INVALID_ARG, "nx and ny must be at least 1");
    const uint64_t nodes = (uint64_t)nx * (uint64_t)ny;
    if (nodes > (uint64_t)OCEAN_GRID_MAX_NODES)
        return fail(OCEAN_E_INVALID_ARG, "nx * ny = " + std::to_string(nodes) + " > OCEAN_GRID_MAX_NODES");
    const size_t want = (size_t)nodes * (mode == OCEAN_GRID_HEIGHTFIELD ? 4 : 32);
    if (bytes != want)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != nx * ny * " +
                                             (mode == OCEAN_GRID_HEIGHTFIELD ? "4 = " : "32 = ") + std::to_string(want));
    return OCEAN_OK;
}

// ... and of the context's state, as the queries.
static int check_grid_state(const ocean_ctx* ctx) {
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_surface_grid");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "surface grid of a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The grid kernel on the ctx stream (device pointer; kind 2 of ocean_kernel_stats).  The workgroup's tile:
// the measured best (docs/MEASUREMENTS.md section 10) unless OCEAN_GRID_TILE names another (A/B).
static int launch_grid(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx,
                       float dz, int nx, int ny, float* d_out) {
    const ocean::DevView v = ctx->view();
    const int tw = ocean::grid_tile_supported(ctx->opt.grid_tile) ? ctx->opt.grid_tile : kGridTileDefault;
    return timed(ctx, 2,
                 [&] {
                     return ocean::launch_surface_grid(v, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, tw, d_out,
                                                       ctx->stream);
                 },
                 "surface_grid");
}

int ocean_surface_grid_device(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                              float dx, float dz, int nx, int ny, float* out, size_t bytes) {
    if (int r = check_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes)) return r;
    // one rule for all modes, though heightfield mode writes one float per node (ocean.h)
    if (int r = check_aligned("ocean_surface_grid_device", nullptr, {}, out)) return r;
    if (int r = check_grid_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return launch_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out);
}

int ocean_surface_grid(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx,
                       float dz, int nx, int ny, float* out, size_t bytes) {
    if (int r = check_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes)) return r;
    if (int r = check_grid_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    // no inputs: the nodes follow from the six numbers
    return run_staged(ctx, "ocean_surface_grid", {}, out, bytes, [&](const float*, float* d_out) {
        return launch_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, d_out);
    });
}

int ocean_surface_grid_async(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                             float dx, float dz, int nx, int ny, float* out, size_t bytes, ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes)) return r;
    // the result is written into a readback slot, whose size start_readback fixes: no points are staged
    const size_t slot_bytes = std::max(ctx->texels() * 16, kQuerySlotBytes);
    if (bytes > slot_bytes)
        return fail(OCEAN_E_INVALID_ARG, "ocean_surface_grid_async: " + std::to_string(bytes) + " B exceed a readback slot of " +
                                             std::to_string(slot_bytes) + " B");
    if (int r = check_grid_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {}, out, bytes,
        [&](const float*, float* d_out) { return launch_grid(ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, d_out); },
        req);
}

// Argument checks of the buoyant bodies, before any device call (ocean.h); `limit`: the forms that stage
// the bodies (host and async) take at most OCEAN_BODY_MAX_BODIES.
static int check_body(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                      const float* bodies, int count, const float* out, bool limit) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!hull || !bodies || !out) return fail(OCEAN_E_INVALID_ARG, "null hull, bodies or output");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    if (mode != OCEAN_QUERY_REFERENCE && mode != OCEAN_QUERY_SURFACE) return fail(OCEAN_E_INVALID_ARG, "unknown query mode");
    if (iterations < 0 || iterations > 16) return fail(OCEAN_E_INVALID_ARG, "iterations must be in [0, 16]");
    if (mode == OCEAN_QUERY_REFERENCE && iterations != 0)
        return fail(OCEAN_E_INVALID_ARG, "OCEAN_QUERY_REFERENCE takes iterations = 0");
    if (probes < 1 || probes > OCEAN_BODY_MAX_PROBES)
        return fail(OCEAN_E_INVALID_ARG, "probes = " + std::to_string(probes) + " outside [1, OCEAN_BODY_MAX_PROBES]");
    if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative body count");
    if (limit && count > OCEAN_BODY_MAX_BODIES)
        return fail(OCEAN_E_INVALID_ARG, "body count " + std::to_string(count) + " > OCEAN_BODY_MAX_BODIES");
    const uint64_t samples = (uint64_t)count * (uint64_t)probes;
    if (samples > (uint64_t)OCEAN_BODY_MAX_SAMPLES)
        return fail(OCEAN_E_INVALID_ARG, "count * probes = " + std::to_string(samples) + " > OCEAN_BODY_MAX_SAMPLES");
    return OCEAN_OK;
}

// ... and of the context's state, as the queries.
static int check_body_state(const ocean_ctx* ctx) {
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_body_buoyancy");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "buoyancy on a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The body kernel on the ctx stream (device pointers; kind 2 of ocean_kernel_stats).
static int launch_body(ocean_ctx* ctx, int tile, int mode, int iterations, const float* d_hull, int probes,
                       const float* d_bodies, int count, float* d_out) {
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] {
                     return ocean::launch_body_buoyancy(v, tile, mode, iterations, d_hull, probes, d_bodies, count, d_out,
                                                        ctx->stream);
                 },
                 "body_buoyancy");
}

// The staged inputs of the host and async forms: the bodies, then the hull right behind them (floats both).
constexpr size_t kBodyInputBytes = (size_t)OCEAN_BODY_MAX_BODIES * 10 * sizeof(float) +
                                   (size_t)OCEAN_BODY_MAX_PROBES * 5 * sizeof(float);
static_assert(kBodyInputBytes <= kQuerySlotBytes - kQueryPointsOffset, "a slot's pinned input copy holds every body request");
static_assert((size_t)OCEAN_BODY_MAX_BODIES * 8 * sizeof(float) <= kQueryPointsOffset, "the records end before the inputs");

int ocean_body_buoyancy_device(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                               const float* bodies, int count, float* out) {
    if (int r = check_body(ctx, tile, mode, iterations, hull, probes, bodies, count, out, false)) return r;
    if (int r = check_aligned("ocean_body_buoyancy_device", "hull and bodies", {hull, bodies}, out)) return r;
    if (int r = check_body_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return launch_body(ctx, tile, mode, iterations, hull, probes, bodies, count, out);
}

int ocean_body_buoyancy(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                        const float* bodies, int count, float* out) {
    if (int r = check_body(ctx, tile, mode, iterations, hull, probes, bodies, count, out, true)) return r;
    if (int r = check_body_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return run_staged(ctx, "ocean_body_buoyancy", {{bodies, (size_t)count * 10 * 4}, {hull, (size_t)probes * 5 * 4}}, out,
                      (size_t)count * 8 * 4, [&](const float* d_in, float* d_out) {
                          return launch_body(ctx, tile, mode, iterations, d_in + (size_t)count * 10, probes, d_in, count, d_out);
                      });
}

int ocean_body_buoyancy_async(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                              const float* bodies, int count, float* out, ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_body(ctx, tile, mode, iterations, hull, probes, bodies, count, out, true)) return r;
    if (count == 0) return fail(OCEAN_E_INVALID_ARG, "ocean_body_buoyancy_async: no bodies, so no request");
    if (int r = check_body_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {{bodies, (size_t)count * 10 * 4}, {hull, (size_t)probes * 5 * 4}}, out, (size_t)count * 8 * 4,
        [&](const float* d_in, float* d_out) {
            return launch_body(ctx, tile, mode, iterations, d_in + (size_t)count * 10, probes, d_in, count, d_out);
        },
        req);
}

// Body dynamics (ocean.h): the checks of the buoyant bodies, then its own two arguments, all before any device
// call; then the context's flag and state, as the velocity queries.
static int check_dynamics(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                          const float* bodies, const float* motion, int count, const float* out, bool limit) {
    if (int r = check_body(ctx, tile, mode, iterations, hull, probes, bodies, count, out, limit)) return r;
    if (!motion) return fail(OCEAN_E_INVALID_ARG, "null motion");
    if (law != OCEAN_DRAG_LINEAR && law != OCEAN_DRAG_QUADRATIC) return fail(OCEAN_E_INVALID_ARG, "unknown drag law");
    return OCEAN_OK;
}

static int check_dynamics_state(const ocean_ctx* ctx) {
    if (!(ctx->flags & OCEAN_F_VELOCITY))
        return fail(OCEAN_E_UNSUPPORTED, "ocean_body_dynamics needs a context created with OCEAN_F_VELOCITY");
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_body_dynamics");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "body dynamics on a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The dynamics kernel on the ctx stream (device pointers; kind 2 of ocean_kernel_stats).
static int launch_dynamics(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* d_hull, int probes,
                           const float* d_bodies, const float* d_motion, int count, float* d_out) {
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] {
                     return ocean::launch_body_dynamics(v, ctx->vel, tile, mode, iterations, law, d_hull, probes, d_bodies,
                                                        d_motion, count, d_out, ctx->stream);
                 },
                 "body_dynamics");
}

// The staged inputs of the host and async forms: the bodies, the motion behind them, then the hull (floats all).
// The async form at the limits: 8192 x 40 B = 320 KiB of bodies + 8192 x 24 B = 192 KiB of motion + 4096 x 20 B =
// 80 KiB of hull = 592 KiB staged, and 8192 x 64 B = 512 KiB of records.  A slot is max(N N 16,
// OCEAN_QUERY_MAX_POINTS 40) >= 2560 KiB, so records and inputs fit it with room to spare (1104 KiB), but not
// in the point queries' layout, whose inputs start at 2048 KiB and have 512 KiB: here the records take the
// slot's first 512 KiB and the inputs follow them at kDynamicsInputOffset, ending at 1104 KiB.
static_assert(kDynamicsInputBytes == 592 * 1024 && kDynamicsInputOffset == 512 * 1024, "the arithmetic above");
static_assert(kDynamicsInputOffset + kDynamicsInputBytes <= kQuerySlotBytes, "records and inputs fit the smallest slot");
static_assert(kDynamicsInputBytes <= kStageInputBytes, "a slot's pinned input copy holds every dynamics request");
static_assert(kDynamicsInputOffset % 16 == 0, "the inputs start float4-aligned");

int ocean_body_dynamics_device(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                               const float* bodies, const float* motion, int count, float* out) {
    if (int r = check_dynamics(ctx, tile, mode, iterations, law, hull, probes, bodies, motion, count, out, false)) return r;
    if (int r = check_aligned("ocean_body_dynamics_device", "hull, bodies and motion", {hull, bodies, motion}, out)) return r;
    if (int r = check_dynamics_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return launch_dynamics(ctx, tile, mode, iterations, law, hull, probes, bodies, motion, count, out);
}

int ocean_body_dynamics(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                        const float* bodies, const float* motion, int count, float* out) {
    if (int r = check_dynamics(ctx, tile, mode, iterations, law, hull, probes, bodies, motion, count, out, true)) return r;
    if (int r = check_dynamics_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return run_staged(ctx, "ocean_body_dynamics",
                      {{bodies, (size_t)count * 10 * 4}, {motion, (size_t)count * 6 * 4}, {hull, (size_t)probes * 5 * 4}}, out,
                      (size_t)count * 16 * 4, [&](const float* d_in, float* d_out) {
                          return launch_dynamics(ctx, tile, mode, iterations, law, d_in + (size_t)count * 16, probes, d_in,
                                                 d_in + (size_t)count * 10, count, d_out);
                      });
}

int ocean_body_dynamics_async(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                              const float* bodies, const float* motion, int count, float* out, ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_dynamics(ctx, tile, mode, iterations, law, hull, probes, bodies, motion, count, out, true)) return r;
    if (count == 0) return fail(OCEAN_E_INVALID_ARG, "ocean_body_dynamics_async: no bodies, so no request");
    if (int r = check_dynamics_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {{bodies, (size_t)count * 10 * 4}, {motion, (size_t)count * 6 * 4}, {hull, (size_t)probes * 5 * 4}}, out,
        (size_t)count * 16 * 4,
        [&](const float* d_in, float* d_out) {
            return launch_dynamics(ctx, tile, mode, iterations, law, d_in + (size_t)count * 16, probes, d_in,
                                   d_in + (size_t)count * 10, count, d_out);
        },
        req, kDynamicsInputOffset);
}

// Surface bounds and ray casts (ocean.h).

// Tile `tile`'s bounds records on the device, float[C][8], current on the ctx stream once this returns: the
// two bounds launches (kind 2 of ocean_kernel_stats) are enqueued unless the cached records still match DISP.
// (the caller has entered: OCEAN_ENTER)
static int ensure_bounds(ocean_ctx* ctx, int tile, const float** records) {
    const size_t rec_floats = ctx->units() * 8;
    if (!ctx->bounds_dev)
        OCEAN_HIP(hipMalloc((void**)&ctx->bounds_dev, (rec_floats + ocean::bounds_partial_floats(ctx->C)) * sizeof(float)));
    float* rec = ctx->bounds_dev + (size_t)tile * ctx->C * 8;
    *records = rec;
    if (ctx->bounds_valid[tile] && !ctx->disp_exposed) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2,
                      [&] { return ocean::launch_surface_bounds(v, tile, ctx->bounds_dev + rec_floats, rec, ctx->stream); },
                      "surface_bounds"))
        return r;
    ctx->bounds_valid[tile] = !ctx->disp_exposed;
    return OCEAN_OK;
}

static int check_bounds(ocean_ctx* ctx, int tile, const float* out, size_t bytes) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    if (bytes != (size_t)ctx->C * 32)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != cascades * 32 = " +
                                             std::to_string((size_t)ctx->C * 32));
    return OCEAN_OK;
}

static int check_bounds_state(const ocean_ctx* ctx) {
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_surface_bounds");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "surface bounds of a column-parity shard (half the columns)");
    return OCEAN_OK;
}

int ocean_surface_bounds_device(ocean_ctx* ctx, int tile, float* out, size_t bytes) {
    if (int r = check_bounds(ctx, tile, out, bytes)) return r;
    if (int r = check_aligned("ocean_surface_bounds_device", nullptr, {}, out)) return r;
    if (int r = check_bounds_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    const float* rec = nullptr;
    if (int r = ensure_bounds(ctx, tile, &rec)) return r;
    OCEAN_HIP(hipMemcpyAsync(out, rec, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return OCEAN_OK;
}

int ocean_surface_bounds(ocean_ctx* ctx, int tile, float* out, size_t bytes) {
    if (int r = check_bounds(ctx, tile, out, bytes)) return r;
    if (int r = check_bounds_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    const float* rec = nullptr;
    if (int r = ensure_bounds(ctx, tile, &rec)) return r;
    OCEAN_HIP(hipMemcpyAsync(out, rec, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

// Argument checks of the ray casts, before any device call (ocean.h); `limit`: the forms that stage the
// rays (host and async) take at most OCEAN_RAY_MAX_RAYS.
static int check_ray(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                     const float* out, bool limit) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!rays || !out) return fail(OCEAN_E_INVALID_ARG, "null rays or output");
    if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative ray count");
    if (limit && count > OCEAN_RAY_MAX_RAYS)
        return fail(OCEAN_E_INVALID_ARG, "ray count " + std::to_string(count) + " > OCEAN_RAY_MAX_RAYS");
    if (steps < 1 || steps > OCEAN_RAY_MAX_STEPS)
        return fail(OCEAN_E_INVALID_ARG, "steps = " + std::to_string(steps) + " outside [1, OCEAN_RAY_MAX_STEPS]");
    const uint64_t samples = (uint64_t)count * (uint64_t)steps;
    if (samples > (uint64_t)OCEAN_RAY_MAX_SAMPLES)
        return fail(OCEAN_E_INVALID_ARG, "count * steps = " + std::to_string(samples) + " > OCEAN_RAY_MAX_SAMPLES");
    if (iterations < 0 || iterations > 16) return fail(OCEAN_E_INVALID_ARG, "iterations must be in [0, 16]");
    if (refine < 0 || refine > 32) return fail(OCEAN_E_INVALID_ARG, "refine must be in [0, 32]");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    return OCEAN_OK;
}

// ... and of the context's state, as the queries.
static int check_ray_state(const ocean_ctx* ctx) {
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_raycast");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "ray cast on a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The ray kernel on the ctx stream (device pointers; kind 2 of ocean_kernel_stats), behind the bounds
// launches where the air skip is on and the tile's bounds are stale.
static int launch_ray(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* d_rays, int count,
                      float* d_out) {
    const float* bounds = nullptr;
    if (ctx->opt.ray_bounds)
        if (int r = ensure_bounds(ctx, tile, &bounds)) return r;
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] {
                     return ocean::launch_raycast(v, tile, iterations, steps, refine, bounds, d_rays, count, d_out,
                                                  ctx->stream);
                 },
                 "raycast");
}

// The staged rays and their records, 32 B each way, fill a slot's two regions exactly.
static_assert((size_t)OCEAN_RAY_MAX_RAYS * 8 * sizeof(float) <= kQuerySlotBytes - kQueryPointsOffset,
              "a slot's pinned input copy holds every ray request");
static_assert((size_t)OCEAN_RAY_MAX_RAYS * 8 * sizeof(float) <= kQueryPointsOffset, "the records end before the inputs");

int ocean_raycast_device(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                         float* out) {
    if (int r = check_ray(ctx, tile, iterations, steps, refine, rays, count, out, false)) return r;
    if (int r = check_aligned("ocean_raycast_device", "rays", {rays}, out)) return r;
    if (int r = check_ray_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return launch_ray(ctx, tile, iterations, steps, refine, rays, count, out);
}

int ocean_raycast(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                  float* out) {
    if (int r = check_ray(ctx, tile, iterations, steps, refine, rays, count, out, true)) return r;
    if (int r = check_ray_state(ctx)) return r;
    if (count == 0) return OCEAN_OK;
    OCEAN_ENTER(ctx);
    return run_staged(ctx, "ocean_raycast", {{rays, (size_t)count * 8 * 4}}, out, (size_t)count * 8 * 4,
                      [&](const float* d_rays, float* d_out) {
                          return launch_ray(ctx, tile, iterations, steps, refine, d_rays, count, d_out);
                      });
}

int ocean_raycast_async(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                        float* dst, ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_ray(ctx, tile, iterations, steps, refine, rays, count, dst, true)) return r;
    if (count == 0) return fail(OCEAN_E_INVALID_ARG, "ocean_raycast_async: no rays, so no request");
    if (int r = check_ray_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {{rays, (size_t)count * 8 * 4}}, dst, (size_t)count * 8 * 4,
        [&](const float* d_rays, float* d_out) {
            return launch_ray(ctx, tile, iterations, steps, refine, d_rays, count, d_out);
        },
        req);
}

// Whitecap emitters (ocean.h).

// Argument checks of the whitecap emitters, before any device call (ocean.h).  What does not need the context
// comes first, so that a host learns of a bad argument whatever its context is; device_out: the _device form's
// output pointer, 16-byte aligned.
static int check_whitecaps(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                           int nx, int ny, int capacity, const float* out, size_t bytes, bool device_out) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
    if (!std::isfinite(lod) || lod < 0.0f) return fail(OCEAN_E_INVALID_ARG, "lod must be finite and >= 0");
    if (!std::isfinite(threshold)) return fail(OCEAN_E_INVALID_ARG, "threshold must be finite");
    if (!std::isfinite(x0) || !std::isfinite(z0) || !std::isfinite(dx) || !std::isfinite(dz))
        return fail(OCEAN_E_INVALID_ARG, "grid origin and spacing must be finite");
    if (nx < 1 || ny < 1) return fail(OCEAN_E_INVALID_ARG, "nx and ny must be at least 1");
    const uint64_t nodes = (uint64_t)nx * (uint64_t)ny;
    if (nodes > (uint64_t)OCEAN_GRID_MAX_NODES)
        return fail(OCEAN_E_INVALID_ARG, "nx * ny = " + std::to_string(nodes) + " > OCEAN_GRID_MAX_NODES");
    if (capacity < 1 || capacity > OCEAN_WHITECAP_MAX_RECORDS)
        return fail(OCEAN_E_INVALID_ARG, "capacity = " + std::to_string(capacity) + " outside [1, OCEAN_WHITECAP_MAX_RECORDS]");
    const size_t want = ((size_t)capacity + 1) * 32;
    if (bytes != want)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != (capacity + 1) * 32 = " +
                                             std::to_string(want));
    if (device_out)
        if (int r = check_aligned("ocean_whitecaps_device", nullptr, {}, out)) return r;
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    return OCEAN_OK;
}

// ... and of the context's flags and state.
static int check_whitecaps_state(const ocean_ctx* ctx) {
    if (ctx->flags & OCEAN_F_DISPLACEMENT_ONLY)
        return fail(OCEAN_E_UNSUPPORTED, "ocean_whitecaps needs the TURB texture (not OCEAN_F_DISPLACEMENT_ONLY)");
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, "ocean_init_spectrum must precede ocean_whitecaps");
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, "whitecaps of a column-parity shard (half the columns)");
    return OCEAN_OK;
}

// The three whitecap kernels on the ctx stream (device pointer; kind 2 of ocean_kernel_stats), over the
// context's scratch, which the first call allocates.  (the caller has entered: OCEAN_ENTER)
static int launch_whitecap_kernels(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx,
                                   float dz, int nx, int ny, int capacity, float* d_out) {
    if (!ctx->whitecap_dev) OCEAN_HIP(hipMalloc(&ctx->whitecap_dev, ocean::whitecap_scratch_bytes()));
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2,
                 [&] {
                     return ocean::launch_whitecaps(v, ctx->vel, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity,
                                                    ctx->whitecap_dev, d_out, ctx->stream);
                 },
                 "whitecaps");
}

// The largest list, header included, fits the smallest readback slot.
static_assert(((size_t)OCEAN_WHITECAP_MAX_RECORDS + 1) * 32 <= kQuerySlotBytes, "a readback slot holds every whitecap list");

int ocean_whitecaps_device(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                           int nx, int ny, int capacity, float* out, size_t bytes) {
    if (int r = check_whitecaps(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes, true)) return r;
    if (int r = check_whitecaps_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return launch_whitecap_kernels(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out);
}

int ocean_whitecaps(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz, int nx,
                    int ny, int capacity, float* out, size_t bytes) {
    if (int r = check_whitecaps(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes, false)) return r;
    if (int r = check_whitecaps_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    // no inputs: the nodes follow from the six numbers
    return run_staged(ctx, "ocean_whitecaps", {}, out, bytes, [&](const float*, float* d_out) {
        return launch_whitecap_kernels(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, d_out);
    });
}

int ocean_whitecaps_async(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                          int nx, int ny, int capacity, float* out, size_t bytes, ocean_readback** req) {
    if (!req) return fail(OCEAN_E_INVALID_ARG, "req is null");
    *req = nullptr;
    if (int r = check_whitecaps(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes, false)) return r;
    if (int r = check_whitecaps_state(ctx)) return r;
    OCEAN_ENTER(ctx);
    return start_staged_readback(
        ctx, {}, out, bytes,
        [&](const float*, float* d_out) {
            return launch_whitecap_kernels(ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, d_out);
        },
        req);
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
