// What the translation units of the C-ABI layer share (abi_context.cpp, abi_frame.cpp, abi_readback.cpp,
// abi_consumers.cpp): the error slot, the context, the device rule of every entry, the launch wrapper of
// kernel timing and the staging of the point consumers.  Not part of the ABI, and except for the context
// itself not visible outside the library.  abi_atmosphere.cpp (the atmosphere's tables) is written over the same.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "device_scope.h"
#include "frame_plan.h"
#include "ocean_internal.h"

// (hidden: shared by the library's translation units, not exported from it)
#pragma GCC visibility push(hidden)
// The calling thread's ocean_last_error (abi_context.cpp) and the code the call returns.
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);
#pragma GCC visibility pop

#define OCEAN_HIP(call)                                   \
    do {                                                  \
        hipError_t _e = (call);                           \
        if (_e != hipSuccess) return hip_fail(_e, #call); \
    } while (0)

// A block of device memory that a context owns and one of its entries sizes: allocated by the first call that
// needs it, grown by free-then-malloc only when a call asks for more than it holds (hipFree waits for the launches
// that still read the old block), never shrunk, and freed by ocean_destroy.  (the caller has entered: OCEAN_ENTER)
struct DeviceScratch {
    void* ptr = nullptr;
    size_t bytes = 0;
    int ensure(size_t need) {
        if (need <= bytes) return OCEAN_OK;
        if (ptr) OCEAN_HIP(hipFree(ptr));
        ptr = nullptr;
        bytes = 0;
        OCEAN_HIP(hipMalloc(&ptr, need));
        bytes = need;
        return OCEAN_OK;
    }
};

struct TimedLaunch {
    int kind;
    hipEvent_t a, b;
};

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
// results, and the pinned copy is sized for it (kStageInputBytes).
constexpr size_t kQueryPointsOffset = (size_t)OCEAN_QUERY_MAX_POINTS * 8 * sizeof(float);
constexpr size_t kQuerySlotBytes = kQueryPointsOffset + (size_t)OCEAN_QUERY_MAX_POINTS * 2 * sizeof(float);
constexpr size_t kDynamicsInputOffset = (size_t)OCEAN_BODY_MAX_BODIES * 16 * sizeof(float);
constexpr size_t kDynamicsInputBytes = (size_t)OCEAN_BODY_MAX_BODIES * (10 + 6) * sizeof(float) +
                                       (size_t)OCEAN_BODY_MAX_PROBES * 5 * sizeof(float);
// ocean_body_step_async outgrows both: its records alone are 1 MiB, so its inputs start at kStepInputOffset, right
// behind them, and it is the largest the pinned copy holds.
constexpr size_t kStepInputOffset = (size_t)OCEAN_BODY_MAX_BODIES * 32 * sizeof(float);
constexpr size_t kStepInputBytes = (size_t)OCEAN_BODY_MAX_BODIES * (32 + 4) * sizeof(float) +
                                   (size_t)OCEAN_BODY_MAX_PROBES * 5 * sizeof(float);
constexpr size_t kStageInputBytes = std::max({kQuerySlotBytes - kQueryPointsOffset, kDynamicsInputBytes, kStepInputBytes});
// What each consumer needs of a slot.  Bodies: the bodies, then the hull right behind them (floats both).
constexpr size_t kBodyInputBytes = (size_t)OCEAN_BODY_MAX_BODIES * 10 * sizeof(float) +
                                   (size_t)OCEAN_BODY_MAX_PROBES * 5 * sizeof(float);
static_assert(kBodyInputBytes <= kQuerySlotBytes - kQueryPointsOffset, "a slot's pinned input copy holds every body request");
static_assert((size_t)OCEAN_BODY_MAX_BODIES * 8 * sizeof(float) <= kQueryPointsOffset, "the records end before the inputs");
// Dynamics: the bodies, the motion behind them, then the hull (floats all).  At the limits: 8192 x 40 B = 320 KiB
// of bodies + 8192 x 24 B = 192 KiB of motion + 4096 x 20 B = 80 KiB of hull = 592 KiB staged, and 8192 x 64 B =
// 512 KiB of records.  A slot is max(N N 16, OCEAN_QUERY_MAX_POINTS 40) >= 2560 KiB, so records and inputs fit it
// with room to spare (1104 KiB), but not in the point queries' layout, whose inputs start at 2048 KiB and have
// 512 KiB: here the records take the slot's first 512 KiB and the inputs follow them at kDynamicsInputOffset,
// ending at 1104 KiB.
static_assert(kDynamicsInputBytes == 592 * 1024 && kDynamicsInputOffset == 512 * 1024, "the arithmetic above");
static_assert(kDynamicsInputOffset + kDynamicsInputBytes <= kQuerySlotBytes, "records and inputs fit the smallest slot");
static_assert(kDynamicsInputBytes <= kStageInputBytes, "a slot's pinned input copy holds every dynamics request");
static_assert(kDynamicsInputOffset % 16 == 0, "the inputs start float4-aligned");
// Steps: the state, the props behind it, then the hull (floats all).  At the limits: 8192 x 128 B = 1024 KiB of state
// + 8192 x 16 B = 128 KiB of props + 80 KiB of hull = 1232 KiB staged, and 8192 x 128 B = 1024 KiB of records, which
// take the slot's first MiB; the inputs follow them at kStepInputOffset and end at 2256 KiB of the smallest slot's 2560.
static_assert(kStepInputBytes == 1232 * 1024 && kStepInputOffset == 1024 * 1024, "the arithmetic above");
static_assert(kQuerySlotBytes == 2560 * 1024, "the smallest slot");
static_assert(kStepInputOffset + kStepInputBytes <= kQuerySlotBytes, "records and inputs fit the smallest slot");
static_assert(kStepInputBytes <= kStageInputBytes, "a slot's pinned input copy holds every step request");
static_assert(kStepInputOffset % 16 == 0, "the inputs start float4-aligned");
// Rays: the staged rays and their records, 32 B each way, fill a slot's two regions exactly.
static_assert((size_t)OCEAN_RAY_MAX_RAYS * 8 * sizeof(float) <= kQuerySlotBytes - kQueryPointsOffset,
              "a slot's pinned input copy holds every ray request");
static_assert((size_t)OCEAN_RAY_MAX_RAYS * 8 * sizeof(float) <= kQueryPointsOffset, "the records end before the inputs");
// Whitecaps: the largest list, header included, fits the smallest slot.  (A surface grid's size depends on its
// arguments: ocean_surface_grid_async checks it against stage_slot_bytes.)
static_assert(((size_t)OCEAN_WHITECAP_MAX_RECORDS + 1) * 32 <= kQuerySlotBytes, "a readback slot holds every whitecap list");
// Spray: the stepped pool, header included, fits the smallest slot like a whitecap list.  Its inputs do not: the pool
// and the emitter list are 2 MiB each at the limits, more than the slot has left and more than the pinned copy
// holds.  ocean_spray_step_async stages them in a block pair of the slot's own (StagedInputs::own_block), which the
// slot's first spray request allocates, so a context that never steps spray holds what it always did.
constexpr size_t kSprayInputBytes = ((size_t)OCEAN_SPRAY_MAX_STAGED + 1) * 32 + ((size_t)OCEAN_WHITECAP_MAX_RECORDS + 1) * 32;
static_assert(((size_t)OCEAN_SPRAY_MAX_STAGED + 1) * 32 <= kQuerySlotBytes, "a readback slot holds every staged pool");
static_assert(kSprayInputBytes == 4096 * 1024, "the arithmetic above");
struct StageSlot {
    void* mem = nullptr;
    void* pts_host = nullptr;    // pinned, kStageInputBytes: the inputs of the request holding the slot
    void* big_host = nullptr;    // pinned, kSprayInputBytes, and its device twin: a spray request's inputs, or the
                                 // bodies of a camera request
    void* big_dev = nullptr;
    hipEvent_t after = nullptr;  // the snapshot is in the slot (the copy stream waits for it)
    hipEvent_t done = nullptr;   // the host copy has landed (untimed requests)
    hipEvent_t tstart = nullptr, tdone = nullptr;  // timed requests: around the host copy itself
};
struct StagePool;  // a context's slots (abi_readback.cpp)

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
    int defer_turb = 1;     // OCEAN_DEFER_TURB=0: pass BQ writes TURB every frame (frame_plan.h defer_turb; A/B)
    int grid_tile = 0;      // OCEAN_GRID_TILE: nodes along x of the grid kernel's workgroup tile, 64 / 32 / 16 (0: kept)
    int vel_nt = 0;         // OCEAN_VEL_NT=1: the velocity pack kernel writes VEL with nontemporal stores
    int prune = 1;          // OCEAN_PRUNE=0: passes AQ / BQ run every row of a band-limited cascade (dense schedule)
    int ray_bounds = 1;     // OCEAN_RAY_BOUNDS=0: the ray kernel samples every node (no air skip, no bounds launches)
    int camera_tile = 1;    // OCEAN_CAMERA_TILE=0: the camera kernel maps pixels to lanes row-linearly, not in 8 x 8 tiles (A/B)
    int camera_cull = 1;    // OCEAN_CAMERA_CULL=0: ocean_camera_bodies* and ocean_camera_scene* hand every body to every tile's slab tests (no cull; A/B)
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
        if (const char* e = std::getenv("OCEAN_DEFER_TURB")) o.defer_turb = std::atoi(e) != 0;
        if (const char* e = std::getenv("OCEAN_GRID_TILE")) o.grid_tile = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_VEL_NT")) o.vel_nt = std::atoi(e) != 0;
        if (const char* e = std::getenv("OCEAN_PRUNE")) o.prune = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_RAY_BOUNDS")) o.ray_bounds = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_CAMERA_TILE")) o.camera_tile = std::atoi(e);
        if (const char* e = std::getenv("OCEAN_CAMERA_CULL")) o.camera_cull = std::atoi(e);
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
    DeviceScratch bounds_dev;
    std::vector<bool> bounds_valid;
    bool disp_exposed = false;
    // deferred TURB (frame_plan.h defer_turb).  turb_stale: a deferred frame has run since the float4 array was
    // last whole, so the foam state is TURB's level 0 and the array waits for materialise_turb.  turb_exposed:
    // ocean_get_device_ptr has handed TURB out, a foreign reader cannot be seen, so every frame writes it, for
    // the life of the context.
    bool turb_stale = false;
    bool turb_exposed = false;
    // whitecap emitters (whitecaps.hip): the ballot masks and per-chunk counts of the largest grid, allocated by the
    // first ocean_whitecaps* call and reused by every later one
    DeviceScratch whitecap_dev;
    // spray particles (spray.hip): the stepped records, ballot masks and per-chunk counts of the largest call so far,
    // allocated by the first ocean_spray_step* call and grown when a call needs more
    DeviceScratch spray_dev;
    // the staging block of the blocking host forms (run_staged_impl): inputs, then the output; grown on demand
    void* stage_block = nullptr;
    size_t stage_block_bytes = 0;
    // the atmosphere (abi_atmosphere.cpp): the three tables in one allocation (`block`: transmittance, multiscatter,
    // sky view, in this order), allocated by ocean_atmosphere and again when its dims change; the params they were
    // made with; sky_valid: the sky view matches them (ocean_sky_update since the last ocean_atmosphere); column: the
    // host copy of column 0 of the transmittance table, float4[h[0]], fetched by the first ocean_sun_color after an
    // ocean_atmosphere
    struct Atmosphere {
        float4* block = nullptr;
        float4* lut[3] = {nullptr, nullptr, nullptr};
        int w[3] = {0, 0, 0}, h[3] = {0, 0, 0};
        ocean::AtmosphereParams params{};
        bool ready = false, sky_valid = false, column_valid = false;
        std::vector<float> column;
        ocean::LutView view(int k) const { return {lut[k], w[k], h[k]}; }
    } atm;
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
                {opt.q, opt.a4, opt.chunk_mib, opt.c4_bands, opt.disp_cached, opt.defer_turb},
                {h0k != nullptr, qside != nullptr, h0k_valid, h0_conj, prune_ready, &prune, turb_exposed}};
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
        v.turb_foam = turb_stale;
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

#pragma GCC visibility push(hidden)

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

// Entry of every call that touches the device: check the context, make its device current until the
// call returns (DeviceScope), or return the failure.
#define OCEAN_ENTER(ctx)                                                        \
    if (!(ctx)) return fail(OCEAN_E_INVALID_ARG, "null context");              \
    DeviceScope device_scope_((ctx)->device);                                   \
    if (const int device_scope_status_ = device_scope_.status()) return device_scope_status_

// Folds timed launches into kind_ms / kind_count and returns their events to the pool (abi_frame.cpp).
// wait: synchronize the stream first (every pending launch is then finished); else fold
// the finished prefix only (stream order: the first unfinished launch ends it).
int fold_pending(ocean_ctx* ctx, bool wait);

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
inline void drop_bounds(ocean_ctx* ctx) { ctx->bounds_valid.assign(ctx->bounds_valid.size(), false); }

// Deferred TURB: the float4 array from the foam state when a deferred frame has left it stale, one launch of
// kind 2 on the context's stream; nothing otherwise (abi_context.cpp).  Every entry that reads, writes or hands
// out the array itself calls it first.
int materialise_turb(ocean_ctx* ctx);

// The address of slice (tile, cascade) of a texture, which must hold `bytes` (abi_context.cpp).
int slice_ptr(ocean_ctx* ctx, int tex, int tile, int cascade, size_t bytes, char** out);

// The staging of the point consumers (abi_readback.cpp); the three forms of a consumer (abi_consumers.cpp:
// device_form, host_form, async_form) are written over it.

// The arrays of the caller's that a consumer's kernel reads, in the order its `launch` takes them.  A host or
// async form stages them back to back in that order (floats all: every offset is 4-byte aligned) and hands
// the launch their device addresses; a _device form hands it the caller's own pointers.
struct HostInput {
    const void* ptr;
    size_t bytes;
};
constexpr int kMaxInputs = 3;
struct StagedInputs {
    const char* names;  // what the _device form's alignment message calls them; null: the consumer has none
    int n;
    HostInput v[kMaxInputs];
    size_t slot_offset = kQueryPointsOffset;  // where an async request puts them in its slot (StageSlot)
    bool own_block = false;  // an async request stages them in the slot's big_host / big_dev pair instead (spray, and
                             // the camera's bodies)
};

// Bytes of a readback slot of this context: the largest slice (float4 textures), or a full surface query's
// points and results (N <= 256).
size_t stage_slot_bytes(const ocean_ctx* ctx);

// The context's staging block (ocean_ctx::stage_block) grows in multiples of this.
constexpr size_t kStageBlockGrain = (size_t)1 << 16;

// A staged launch: (device addresses of the inputs, device address of the output) -> an OCEAN_* code.  Passed
// as a plain function and its argument: these calls are latency-bound, nothing here allocates.
using StagedLaunch = int (*)(const void* arg, const float* const* d_in, float* d_out);
int run_staged_impl(ocean_ctx* ctx, const char* entry, const StagedInputs& in, void* out, size_t out_bytes,
                    StagedLaunch launch, const void* arg);
int start_staged_readback_impl(ocean_ctx* ctx, const StagedInputs& in, void* dst, size_t out_bytes, StagedLaunch launch,
                               const void* arg, ocean_readback** req);
template <class F>
int call_staged(const void* f, const float* const* d_in, float* d_out) {
    return (*static_cast<const F*>(f))(d_in, d_out);
}
// The blocking host form: upload, launch, download, synchronize, through the context's staging block.
template <class F>
int run_staged(ocean_ctx* ctx, const char* entry, const StagedInputs& in, void* out, size_t out_bytes, const F& launch) {
    return run_staged_impl(ctx, entry, in, out, out_bytes, &call_staged<F>, &launch);
}
// The async form: a readback request whose snapshot is the kernel's result.
template <class F>
int start_staged_readback(ocean_ctx* ctx, const StagedInputs& in, void* dst, size_t out_bytes, const F& launch,
                          ocean_readback** req) {
    return start_staged_readback_impl(ctx, in, dst, out_bytes, &call_staged<F>, &launch, req);
}

#pragma GCC visibility pop

