// C-ABI layer of liboceanhip.so, the readback requests: the pool of staging slots (abi_internal.h has a slot's
// layout), the requests' entries, and the staging of the point consumers' host and async forms.
#include <mutex>
#include <new>

#include "abi_internal.h"

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
            if (sl->big_host) (void)hipHostFree(sl->big_host);
            if (sl->big_dev) (void)hipFree(sl->big_dev);
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
// `snapshot` returns an OCEAN_* code, the failing call's own message set.
template <class Snapshot>
int start_readback(ocean_ctx* ctx, void* dst, size_t bytes, Snapshot&& snapshot, ocean_readback** out) {
    if (!ctx->copy_stream) OCEAN_HIP(hipStreamCreateWithFlags(&ctx->copy_stream, hipStreamNonBlocking));
    if (!ctx->stage_pool) {
        ctx->stage_pool = std::make_shared<StagePool>();
        ctx->stage_pool->device = ctx->device;
        ctx->stage_pool->slot_bytes = stage_slot_bytes(ctx);
    }
    ocean_readback* rb = new (std::nothrow) ocean_readback();
    if (!rb) return fail(OCEAN_E_OUT_OF_MEMORY, "host allocation failed");
    rb->device = ctx->device;
    rb->pool = ctx->stage_pool;
    rb->timed = ctx->readback_timing;
    hipError_t e = rb->pool->take(rb->timed, &rb->slot);
    const int r = e == hipSuccess ? snapshot(rb->slot) : OCEAN_OK;
    if (r == OCEAN_OK) {
        if (e == hipSuccess) e = hipEventRecord(rb->slot->after, ctx->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(ctx->copy_stream, rb->slot->after, 0);
        if (e == hipSuccess && rb->timed) e = hipEventRecord(rb->slot->tstart, ctx->copy_stream);
        if (e == hipSuccess) e = hipMemcpyAsync(dst, rb->slot->mem, bytes, kReadbackCopyKind, ctx->copy_stream);
        if (e == hipSuccess) e = hipEventRecord(rb->done(), ctx->copy_stream);
    }
    if (r != OCEAN_OK || e != hipSuccess) {
        (void)hipStreamSynchronize(ctx->copy_stream);
        (void)hipStreamSynchronize(ctx->stream);
        if (rb->slot) rb->pool->give(rb->slot);
        delete rb;
        return r != OCEAN_OK ? r : hip_fail(e, "readback request");
    }
    *out = rb;
    return OCEAN_OK;
}
}  // namespace

size_t stage_slot_bytes(const ocean_ctx* ctx) { return std::max(ctx->texels() * 16, kQuerySlotBytes); }

// The blocking host form: one block of device memory that the context owns (stage_block: hipMalloc, grown on
// demand, freed by ocean_destroy) holds the inputs from its base and the output at the next 256-byte boundary
// (float4 output rows stay 16-B aligned); upload, launch, download, synchronize.  The call ends with the stream
// idle, so the block is free again when the next blocking call starts, and growing it frees nothing in use.
// It was a stream-ordered block per call (hipMallocAsync before the upload, hipFreeAsync behind the download) until
// tests/test_gpu_host_sequences.py played sequences of blocking calls in one process on the system's HIP runtime
// (/opt/rocm 7.2.0): the results of ocean_camera, ocean_whitecaps and ocean_surface_grid came back all zero or
// partly written, and those of ocean_query_surface and ocean_sample_world with wrong numbers, each with OCEAN_OK
// and from a compiled host and a torch-less Python alike, while the same calls on the runtime torch bundles were
// right (docs/MEASUREMENTS.md section 24).  What in the runtime differs was not looked for.
// The launch's own code comes first, then the copies' and the synchronize's.
int run_staged_impl(ocean_ctx* ctx, const char* entry, const StagedInputs& in, void* out, size_t out_bytes,
                    StagedLaunch launch, const void* arg) {
    size_t in_bytes = 0;
    for (int k = 0; k < in.n; ++k) in_bytes += in.v[k].bytes;
    const size_t out_off = (in_bytes + 255) & ~(size_t)255;
    const size_t need = out_off + out_bytes;
    if (need > ctx->stage_block_bytes) {
        if (ctx->stage_block) OCEAN_HIP(hipFree(ctx->stage_block));
        ctx->stage_block = nullptr;
        ctx->stage_block_bytes = 0;
        const size_t bytes = (need + kStageBlockGrain - 1) / kStageBlockGrain * kStageBlockGrain;
        OCEAN_HIP(hipMalloc(&ctx->stage_block, bytes));
        ctx->stage_block_bytes = bytes;
    }
    char* base = static_cast<char*>(ctx->stage_block);
    float* d_out = reinterpret_cast<float*>(base + out_off);
    const float* d_in[kMaxInputs] = {};
    hipError_t e = hipSuccess;
    size_t off = 0;
    for (int k = 0; k < in.n; ++k) {
        d_in[k] = reinterpret_cast<const float*>(base + off);
        if (e == hipSuccess) e = hipMemcpyAsync(base + off, in.v[k].ptr, in.v[k].bytes, hipMemcpyHostToDevice, ctx->stream);
        off += in.v[k].bytes;
    }
    int r = OCEAN_OK;
    if (e == hipSuccess) r = launch(arg, d_in, d_out);
    if (e == hipSuccess && r == OCEAN_OK) e = hipMemcpyAsync(out, d_out, out_bytes, hipMemcpyDeviceToHost, ctx->stream);
    const hipError_t es = hipStreamSynchronize(ctx->stream);
    if (r != OCEAN_OK) return r;
    if (e != hipSuccess) return hip_fail(e, (std::string(entry) + " copy").c_str());
    if (es != hipSuccess) return hip_fail(es, "hipStreamSynchronize");
    return OCEAN_OK;
}

// The async form, a readback request whose snapshot is the kernel's result (StageSlot has the layout): the
// caller's inputs are consumed here, into the pinned memory the slot owns, so the one upload that carries
// them all is truly asynchronous and reads nothing of the caller's after this call returns; the kernel
// then writes its results at the slot's base.
int start_staged_readback_impl(ocean_ctx* ctx, const StagedInputs& in, void* dst, size_t out_bytes, StagedLaunch launch,
                               const void* arg, ocean_readback** req) {
    return start_readback(
        ctx, dst, out_bytes,
        [&](StageSlot* sl) -> int {
            char* base = static_cast<char*>(sl->mem) + in.slot_offset;
            void* host = nullptr;
            const float* d_in[kMaxInputs] = {};
            if (in.n != 0 && in.own_block) {  // inputs that outgrow the slot: its own block pair
                if (!sl->big_host) OCEAN_HIP(hipHostMalloc(&sl->big_host, kSprayInputBytes, hipHostMallocDefault));
                if (!sl->big_dev) OCEAN_HIP(hipMalloc(&sl->big_dev, kSprayInputBytes));
                base = static_cast<char*>(sl->big_dev);
                host = sl->big_host;
            } else if (in.n != 0) {
                if (!sl->pts_host) OCEAN_HIP(hipHostMalloc(&sl->pts_host, kStageInputBytes, hipHostMallocDefault));
                host = sl->pts_host;
            }
            if (in.n != 0) {
                size_t in_bytes = 0;
                for (int k = 0; k < in.n; ++k) {
                    d_in[k] = reinterpret_cast<const float*>(base + in_bytes);
                    std::memcpy(static_cast<char*>(host) + in_bytes, in.v[k].ptr, in.v[k].bytes);
                    in_bytes += in.v[k].bytes;
                }
                OCEAN_HIP(hipMemcpyAsync(base, host, in_bytes, hipMemcpyHostToDevice, ctx->stream));
            }
            return launch(arg, d_in, static_cast<float*>(sl->mem));
        },
        req);
}

extern "C" {

int ocean_read_async(ocean_ctx* ctx, int texture, int tile, int cascade, void* dst, size_t bytes,
                     ocean_readback** out) {
    if (!out) return fail(OCEAN_E_INVALID_ARG, "out is null");
    *out = nullptr;
    OCEAN_ENTER(ctx);
    if (!dst) return fail(OCEAN_E_INVALID_ARG, "null destination");
    char* src = nullptr;
    if (int r = slice_ptr(ctx, texture, tile, cascade, bytes, &src)) return r;
    if (texture == OCEAN_TEX_TURB)  // deferred TURB: the array from the foam state first
        if (int r = materialise_turb(ctx)) return r;
    return start_readback(
        ctx, dst, bytes,
        [&](StageSlot* sl) -> int {
            OCEAN_HIP(hipMemcpyAsync(sl->mem, src, bytes, hipMemcpyDeviceToDevice, ctx->stream));
            return OCEAN_OK;
        },
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
        [&](StageSlot* sl) -> int {
            OCEAN_HIP(ocean::launch_extract_height(reinterpret_cast<const float4*>(src), static_cast<float*>(sl->mem),
                                                   ctx->texels(), ctx->stream));
            return OCEAN_OK;
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

}  // extern "C"
