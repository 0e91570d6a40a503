// C-ABI layer of liboceanhip.so, the point consumers (ocean.h): surface and velocity queries, surface grids,
// buoyant bodies, body dynamics, body steps, mesh hulls, ray casts, whitecap emitters, spray particles and camera views (without
// the bodies, with them, and with the water seeing them), each in a _device, a blocking host
// and an _async form; and world sampling and the surface bounds, which keep bodies of their own.
//
// A consumer is stated once, as a struct built from its entry's arguments (a "family"), and its three entries
// are the three forms of that struct: device_form, host_form, async_form.  A family has
//   ctx, out          the context and the caller's output pointer;
//   check(form)       its argument checks, before any device call.  They take the form because the staged forms
//                     (host and async) have a limit on what they stage, and a family may place its alignment
//                     or slot-size test among its own;
//   state()           what it needs of the context (StateRule);
//   inputs()          the caller's arrays its kernel reads (StagedInputs), in the order launch takes them;
//   out_bytes()       the size of its results;
//   lacks()           null, or the noun of what an empty call has none of ("points"): the blocking forms then
//                     return OCEAN_OK without a launch, and the async form refuses, since there is no request;
//   launch(in, out)   its kernel on the ctx stream over device pointers (kind 2 of ocean_kernel_stats), the
//                     caller having entered the device scope.
// The order of the tests of each form is the form's, below, and the same for every family.
#include <algorithm>
#include <cmath>

#include "abi_internal.h"

namespace {

enum class Form { Device, Host, Async };

// What a family needs of its context: the flag it was created with or without, the spectrum (the cascade
// wavelengths exist only after init), and all the columns (a column-parity shard holds half of them).
enum class Needs { Nothing, Velocity, Turb };
struct StateRule {
    const char* entry;  // the family's name in messages, and the stem of its entries' names
    const char* shard;  // "surface query of": ... a column-parity shard
    Needs needs = Needs::Nothing;
    bool sky = false;  // it reads the sky-view table, which must be there and current (ocean_sky_update)
};
int check_state(const ocean_ctx* ctx, const StateRule& s) {
    if (s.needs == Needs::Velocity && !(ctx->flags & OCEAN_F_VELOCITY))
        return fail(OCEAN_E_UNSUPPORTED, std::string(s.entry) + " needs a context created with OCEAN_F_VELOCITY");
    if (s.needs == Needs::Turb && (ctx->flags & OCEAN_F_DISPLACEMENT_ONLY))
        return fail(OCEAN_E_UNSUPPORTED, std::string(s.entry) + " needs the TURB texture (not OCEAN_F_DISPLACEMENT_ONLY)");
    if (!ctx->spectrum_ready) return fail(OCEAN_E_STATE, std::string("ocean_init_spectrum must precede ") + s.entry);
    if (ctx->col_par >= 0) return fail(OCEAN_E_UNSUPPORTED, std::string(s.shard) + " a column-parity shard (half the columns)");
    if (s.sky && !(ctx->atm.ready && ctx->atm.sky_valid))
        return fail(OCEAN_E_STATE, std::string(s.entry) + " with OCEAN_CAMERA_SKY_LUT needs ocean_atmosphere and an ocean_sky_update after it");
    return OCEAN_OK;
}

// The _device forms: the kernels read floats and write float4 rows (ocean.h).
int check_aligned(const char* entry, const StagedInputs& in, const void* out) {
    bool ok = ((uintptr_t)out & 15) == 0;
    for (int k = 0; k < in.n; ++k) ok = ok && ((uintptr_t)in.v[k].ptr & 3) == 0;
    if (ok) return OCEAN_OK;
    return fail(OCEAN_E_INVALID_ARG, std::string(entry) + "_device: " +
                                         (in.names ? std::string(in.names) + " must be 4-byte and out" : "out must be") +
                                         " 16-byte aligned");
}

int check_tile(const ocean_ctx* ctx, int tile) {
    if (tile < 0 || tile >= ctx->T) return fail(OCEAN_E_INVALID_ARG, "tile out of range");
    return OCEAN_OK;
}

int check_iterations(int iterations) {
    if (iterations < 0 || iterations > 16) return fail(OCEAN_E_INVALID_ARG, "iterations must be in [0, 16]");
    return OCEAN_OK;
}

// A mode of the `what` ("query", "grid") modes, and its iterations: none in the mode `direct`, which takes no
// fixed-point steps.
int check_mode(bool known, const char* what, int iterations, bool is_direct, const char* direct) {
    if (!known) return fail(OCEAN_E_INVALID_ARG, std::string("unknown ") + what + " mode");
    if (int r = check_iterations(iterations)) return r;
    if (is_direct && iterations != 0) return fail(OCEAN_E_INVALID_ARG, std::string(direct) + " takes iterations = 0");
    return OCEAN_OK;
}
int check_query_mode(int mode, int iterations) {
    return check_mode(mode == OCEAN_QUERY_REFERENCE || mode == OCEAN_QUERY_SURFACE, "query", iterations,
                      mode == OCEAN_QUERY_REFERENCE, "OCEAN_QUERY_REFERENCE");
}

// The region of a grid: nx x ny nodes from (x0, z0), (dx, dz) apart.
int check_region(float x0, float z0, float dx, float dz, int nx, int ny) {
    if (!std::isfinite(x0) || !std::isfinite(z0) || !std::isfinite(dx) || !std::isfinite(dz))
        return fail(OCEAN_E_INVALID_ARG, "grid origin and spacing must be finite");
    if (nx < 1 || ny < 1) return fail(OCEAN_E_INVALID_ARG, "nx and ny must be at least 1");
    const uint64_t nodes = (uint64_t)nx * (uint64_t)ny;
    if (nodes > (uint64_t)OCEAN_GRID_MAX_NODES)
        return fail(OCEAN_E_INVALID_ARG, "nx * ny = " + std::to_string(nodes) + " > OCEAN_GRID_MAX_NODES");
    return OCEAN_OK;
}

// The _device form: the caller's own device pointers go to the launch; nothing is staged, so no limit.
template <class Family>
int device_form(const Family& f) {
    if (int r = f.check(Form::Device)) return r;
    const StagedInputs in = f.inputs();
    if (int r = check_aligned(f.state().entry, in, f.out)) return r;
    if (int r = check_state(f.ctx, f.state())) return r;
    if (f.lacks()) return OCEAN_OK;
    OCEAN_ENTER(f.ctx);
    const float* d_in[kMaxInputs] = {};
    for (int k = 0; k < in.n; ++k) d_in[k] = static_cast<const float*>(in.v[k].ptr);
    return f.launch(d_in, f.out);
}

// The blocking host form: inputs and results through the context's staging block (run_staged).
template <class Family>
int host_form(const Family& f) {
    if (int r = f.check(Form::Host)) return r;
    if (int r = check_state(f.ctx, f.state())) return r;
    if (f.lacks()) return OCEAN_OK;
    OCEAN_ENTER(f.ctx);
    return run_staged(f.ctx, f.state().entry, f.inputs(), f.out, f.out_bytes(),
                      [&](const float* const* d_in, float* d_out) { return f.launch(d_in, d_out); });
}

// The async form: a readback request over a slot (start_staged_readback).  req_name: the parameter's name in
// ocean.h.
template <class Family>
int async_form(const Family& f, ocean_readback** req, const char* req_name = "req") {
    if (!req) return fail(OCEAN_E_INVALID_ARG, std::string(req_name) + " is null");
    *req = nullptr;
    if (int r = f.check(Form::Async)) return r;
    if (const char* noun = f.lacks())
        return fail(OCEAN_E_INVALID_ARG, std::string(f.state().entry) + "_async: no " + noun + ", so no request");
    if (int r = check_state(f.ctx, f.state())) return r;
    OCEAN_ENTER(f.ctx);
    return start_staged_readback(f.ctx, f.inputs(), f.out, f.out_bytes(),
                                 [&](const float* const* d_in, float* d_out) { return f.launch(d_in, d_out); }, req);
}

// Surface queries: points float[count][2] -> records float[count][8]; the staged forms take at most
// OCEAN_QUERY_MAX_POINTS.
struct SurfaceQuery {
    ocean_ctx* ctx;
    int tile, mode, iterations;
    const float* points;
    int count;
    float* out;

    int check(Form form) const {
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        if (!points || !out) return fail(OCEAN_E_INVALID_ARG, "null points or output");
        if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative point count");
        if (form != Form::Device && count > OCEAN_QUERY_MAX_POINTS)
            return fail(OCEAN_E_INVALID_ARG, "point count " + std::to_string(count) + " > OCEAN_QUERY_MAX_POINTS");
        if (int r = check_query_mode(mode, iterations)) return r;
        return check_tile(ctx, tile);
    }
    StateRule state() const { return {"ocean_query_surface", "surface query of"}; }
    StagedInputs inputs() const { return {"points", 1, {{points, (size_t)count * 2 * 4}}}; }
    size_t out_bytes() const { return (size_t)count * 8 * 4; }
    const char* lacks() const { return count == 0 ? "points" : nullptr; }
    int launch(const float* const* in, float* d_out) const {
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] { return ocean::launch_query_surface(v, tile, mode, iterations, in[0], count, d_out, ctx->stream); },
                     "query_surface");
    }
};

// Surface-velocity queries: the surface query in surface mode, over the VELOCITY texture.
struct VelocityQuery : SurfaceQuery {
    StateRule state() const { return {"ocean_query_velocity", "velocity query of", Needs::Velocity}; }
    int launch(const float* const* in, float* d_out) const {
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] { return ocean::launch_query_velocity(v, ctx->vel, tile, iterations, in[0], count, d_out, ctx->stream); },
                     "query_velocity");
    }
};

// Workgroup tile of the grid kernel (grid.hip), nodes along x: the fastest of the shapes measured
// (docs/MEASUREMENTS.md section 10) unless OCEAN_GRID_TILE names another (A/B).
constexpr int kGridTileDefault = 32;

// Surface grids: no inputs, the nodes follow from the six numbers; float[ny][nx][8], or float[ny][nx] in
// heightfield mode.  One alignment rule for all modes, though heightfield mode writes one float per node.
struct SurfaceGrid {
    ocean_ctx* ctx;
    int tile, mode, iterations;
    float lod, x0, z0, dx, dz;
    int nx, ny;
    float* out;
    size_t bytes;

    int check(Form form) const {
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
        if (int r = check_tile(ctx, tile)) return r;
        if (int r = check_mode(mode == OCEAN_GRID_VERTICES || mode == OCEAN_GRID_SURFACE || mode == OCEAN_GRID_HEIGHTFIELD,
                               "grid", iterations, mode == OCEAN_GRID_VERTICES, "OCEAN_GRID_VERTICES"))
            return r;
        if (!std::isfinite(lod) || lod < 0.0f) return fail(OCEAN_E_INVALID_ARG, "lod must be finite and >= 0");
        if (mode != OCEAN_GRID_VERTICES && lod != 0.0f)
            return fail(OCEAN_E_INVALID_ARG, "OCEAN_GRID_SURFACE and OCEAN_GRID_HEIGHTFIELD take lod = 0");
        if (int r = check_region(x0, z0, dx, dz, nx, ny)) return r;
        const size_t want = (size_t)nx * (size_t)ny * (mode == OCEAN_GRID_HEIGHTFIELD ? 4 : 32);
        if (bytes != want)
            return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != nx * ny * " +
                                                 (mode == OCEAN_GRID_HEIGHTFIELD ? "4 = " : "32 = ") + std::to_string(want));
        // the async form's result is written into a readback slot
        if (form == Form::Async && bytes > stage_slot_bytes(ctx))
            return fail(OCEAN_E_INVALID_ARG, "ocean_surface_grid_async: " + std::to_string(bytes) +
                                                 " B exceed a readback slot of " + std::to_string(stage_slot_bytes(ctx)) + " B");
        return OCEAN_OK;
    }
    StateRule state() const { return {"ocean_surface_grid", "surface grid of"}; }
    StagedInputs inputs() const { return {nullptr, 0, {}}; }
    size_t out_bytes() const { return bytes; }
    const char* lacks() const { return nullptr; }
    int launch(const float* const*, float* d_out) const {
        const ocean::DevView v = ctx->view();
        const int tw = ocean::grid_tile_supported(ctx->opt.grid_tile) ? ctx->opt.grid_tile : kGridTileDefault;
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_surface_grid(v, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, tw, d_out,
                                                           ctx->stream);
                     },
                     "surface_grid");
    }
};

// Buoyant bodies: bodies float[count][10] and the hull float[probes][5] -> records float[count][8]; the staged
// forms take at most OCEAN_BODY_MAX_BODIES.
struct BodyBuoyancy {
    ocean_ctx* ctx;
    int tile, mode, iterations;
    const float* hull;
    int probes;
    const float* bodies;
    int count;
    float* out;

    int check(Form form) const {
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        if (!hull || !bodies || !out) return fail(OCEAN_E_INVALID_ARG, "null hull, bodies or output");
        if (int r = check_tile(ctx, tile)) return r;
        if (int r = check_query_mode(mode, iterations)) return r;
        if (probes < 1 || probes > OCEAN_BODY_MAX_PROBES)
            return fail(OCEAN_E_INVALID_ARG, "probes = " + std::to_string(probes) + " outside [1, OCEAN_BODY_MAX_PROBES]");
        if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative body count");
        if (form != Form::Device && count > OCEAN_BODY_MAX_BODIES)
            return fail(OCEAN_E_INVALID_ARG, "body count " + std::to_string(count) + " > OCEAN_BODY_MAX_BODIES");
        const uint64_t samples = (uint64_t)count * (uint64_t)probes;
        if (samples > (uint64_t)OCEAN_BODY_MAX_SAMPLES)
            return fail(OCEAN_E_INVALID_ARG, "count * probes = " + std::to_string(samples) + " > OCEAN_BODY_MAX_SAMPLES");
        return OCEAN_OK;
    }
    StateRule state() const { return {"ocean_body_buoyancy", "buoyancy on"}; }
    StagedInputs inputs() const {
        return {"hull and bodies", 2, {{bodies, (size_t)count * 10 * 4}, {hull, (size_t)probes * 5 * 4}}};
    }
    size_t out_bytes() const { return (size_t)count * 8 * 4; }
    const char* lacks() const { return count == 0 ? "bodies" : nullptr; }
    int launch(const float* const* in, float* d_out) const {
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_body_buoyancy(v, tile, mode, iterations, in[1], probes, in[0], count, d_out,
                                                            ctx->stream);
                     },
                     "body_buoyancy");
    }
};

// Body dynamics: the buoyant bodies with their motion float[count][6] and a drag law -> records float[count][16].
// Its inputs outgrow the point queries' place in a slot (StageSlot), so they start behind its own records.
struct BodyDynamics : BodyBuoyancy {
    int law;
    const float* motion;

    int check(Form form) const {
        if (int r = BodyBuoyancy::check(form)) return r;
        if (!motion) return fail(OCEAN_E_INVALID_ARG, "null motion");
        if (law != OCEAN_DRAG_LINEAR && law != OCEAN_DRAG_QUADRATIC) return fail(OCEAN_E_INVALID_ARG, "unknown drag law");
        return OCEAN_OK;
    }
    StateRule state() const { return {"ocean_body_dynamics", "body dynamics on", Needs::Velocity}; }
    StagedInputs inputs() const {
        return {"hull, bodies and motion",
                3,
                {{bodies, (size_t)count * 10 * 4}, {motion, (size_t)count * 6 * 4}, {hull, (size_t)probes * 5 * 4}},
                kDynamicsInputOffset};
    }
    size_t out_bytes() const { return (size_t)count * 16 * 4; }
    int launch(const float* const* in, float* d_out) const {
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_body_dynamics(v, ctx->vel, tile, mode, iterations, law, in[2], probes, in[0],
                                                            in[1], count, d_out, ctx->stream);
                     },
                     "body_dynamics");
    }
};

// Body steps: the state float[count][32] (in the place of the bodies), the props float[count][4] and the hull, with
// the eight `step` floats by value -> the stepped state and the last substep's record, float[count][32].  Its records
// alone fill a MiB of a slot, so its inputs start behind them (StageSlot).  The _device form may be given out == state.
struct BodyStep : BodyBuoyancy {
    int law, substeps;
    const float* step;
    const float* props;

    // Its own arguments first, none of which needs the context (as the camera's: a host learns of a bad argument
    // whatever its context is), then everything the bodies refuse.
    int check(Form form) const {
        if (!step || !props || !bodies) return fail(OCEAN_E_INVALID_ARG, "null step, props or state");
        if (law != OCEAN_DRAG_LINEAR && law != OCEAN_DRAG_QUADRATIC) return fail(OCEAN_E_INVALID_ARG, "unknown drag law");
        for (int k = 0; k < OCEAN_BODY_STEP_FLOATS; ++k)
            if (!std::isfinite(step[k])) return fail(OCEAN_E_INVALID_ARG, "step[" + std::to_string(k) + "] is not finite");
        if (substeps < 1 || substeps > OCEAN_BODY_MAX_SUBSTEPS)
            return fail(OCEAN_E_INVALID_ARG, "substeps = " + std::to_string(substeps) + " outside [1, OCEAN_BODY_MAX_SUBSTEPS]");
        if (count > 0 && probes > 0) {
            const uint64_t samples = (uint64_t)count * (uint64_t)probes * (uint64_t)substeps;
            if (samples > (uint64_t)OCEAN_BODY_STEP_MAX_SAMPLES)
                return fail(OCEAN_E_INVALID_ARG, "count * probes * substeps = " + std::to_string(samples) +
                                                     " > OCEAN_BODY_STEP_MAX_SAMPLES");
        }
        return BodyBuoyancy::check(form);
    }
    StateRule state() const { return {"ocean_body_step", "body steps on", Needs::Velocity}; }
    StagedInputs inputs() const {
        return {"hull, props and state",
                3,
                {{bodies, (size_t)count * 32 * 4}, {props, (size_t)count * 4 * 4}, {hull, (size_t)probes * 5 * 4}},
                kStepInputOffset};
    }
    size_t out_bytes() const { return (size_t)count * 32 * 4; }
    int launch(const float* const* in, float* d_out) const {
        ocean::BodyStepParams sp;
        std::copy(step, step + OCEAN_BODY_STEP_FLOATS, sp.p);
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_body_step(v, ctx->vel, tile, mode, iterations, law, substeps, sp, in[2], probes,
                                                        in[1], in[0], count, d_out, ctx->stream);
                     },
                     "body_step");
    }
};

// Mesh hulls: bodies float[count][10], vertices float[nverts][3] and triangles int[ntris][3] -> records
// float[count][16]; always in surface mode.  Its own arguments first, none of which needs the context (as the body
// steps': a host learns of a bad argument whatever its context is), the _device form's alignment and the staged forms'
// look at the indices among them; then the context and the tile.  At the limits the staged forms carry 320 KiB of
// bodies, 24 KiB of vertices and 48 KiB of indices in, and 512 KiB of records out: the point queries' place in a slot.
struct BodyHydrostatics {
    ocean_ctx* ctx;
    int tile, iterations;
    const float* vertices;
    int nverts;
    const int* triangles;
    int ntris;
    const float* bodies;
    int count;
    float* out;

    int check(Form form) const {
        if (!vertices || !triangles || !bodies || !out)
            return fail(OCEAN_E_INVALID_ARG, "null vertices, triangles, bodies or output");
        if (int r = check_iterations(iterations)) return r;
        if (nverts < 1 || nverts > OCEAN_HULL_MAX_VERTICES)
            return fail(OCEAN_E_INVALID_ARG, "nverts = " + std::to_string(nverts) + " outside [1, OCEAN_HULL_MAX_VERTICES]");
        if (ntris < 1 || ntris > OCEAN_HULL_MAX_TRIANGLES)
            return fail(OCEAN_E_INVALID_ARG, "ntris = " + std::to_string(ntris) + " outside [1, OCEAN_HULL_MAX_TRIANGLES]");
        if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative body count");
        if (form != Form::Device && count > OCEAN_BODY_MAX_BODIES)
            return fail(OCEAN_E_INVALID_ARG, "body count " + std::to_string(count) + " > OCEAN_BODY_MAX_BODIES");
        const uint64_t samples = (uint64_t)count * (uint64_t)nverts;
        if (samples > (uint64_t)OCEAN_BODY_MAX_SAMPLES)
            return fail(OCEAN_E_INVALID_ARG, "count * nverts = " + std::to_string(samples) + " > OCEAN_BODY_MAX_SAMPLES");
        if (form == Form::Device) {
            if (int r = check_aligned(state().entry, inputs(), out)) return r;
        } else {  // the staged forms see the indices; the device form's kernel clamps them
            for (size_t k = 0; k < (size_t)ntris * 3; ++k)
                if (triangles[k] < 0 || triangles[k] >= nverts)
                    return fail(OCEAN_E_INVALID_ARG, "triangles[" + std::to_string(k / 3) + "][" + std::to_string(k % 3) +
                                                         "] = " + std::to_string(triangles[k]) + " outside [0, nverts)");
        }
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        return check_tile(ctx, tile);
    }
    StateRule state() const { return {"ocean_body_hydrostatics", "hydrostatics on"}; }
    StagedInputs inputs() const {
        return {"vertices, triangles and bodies",
                3,
                {{bodies, (size_t)count * 10 * 4}, {vertices, (size_t)nverts * 3 * 4}, {triangles, (size_t)ntris * 3 * 4}}};
    }
    size_t out_bytes() const { return (size_t)count * OCEAN_HULL_RECORD_FLOATS * 4; }
    const char* lacks() const { return count == 0 ? "bodies" : nullptr; }
    int launch(const float* const* in, float* d_out) const {
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_body_hydrostatics(v, tile, iterations, in[1], nverts,
                                                                reinterpret_cast<const int*>(in[2]), ntris, in[0], count,
                                                                d_out, ctx->stream);
                     },
                     "body_hydrostatics");
    }
};
static_assert((size_t)OCEAN_BODY_MAX_BODIES * 10 * 4 + (size_t)OCEAN_HULL_MAX_VERTICES * 3 * 4 +
                      (size_t)OCEAN_HULL_MAX_TRIANGLES * 3 * 4 <= kQuerySlotBytes - kQueryPointsOffset,
              "a slot's pinned input copy holds every hydrostatics request");
static_assert((size_t)OCEAN_BODY_MAX_BODIES * OCEAN_HULL_RECORD_FLOATS * 4 <= kQueryPointsOffset,
              "the records end before the inputs");

// Tile `tile`'s bounds records on the device, float[C][8], current on the ctx stream once this returns: the
// two bounds launches (kind 2 of ocean_kernel_stats) are enqueued unless the cached records still match DISP.
// (the caller has entered: OCEAN_ENTER)
int ensure_bounds(ocean_ctx* ctx, int tile, const float** records) {
    const size_t rec_floats = ctx->units() * 8;
    if (int r = ctx->bounds_dev.ensure((rec_floats + ocean::bounds_partial_floats(ctx->C)) * sizeof(float))) return r;
    float* base = static_cast<float*>(ctx->bounds_dev.ptr);
    float* rec = base + (size_t)tile * ctx->C * 8;
    *records = rec;
    if (ctx->bounds_valid[tile] && !ctx->disp_exposed) return OCEAN_OK;
    const ocean::DevView v = ctx->view();
    if (int r = timed(ctx, 2,
                      [&] { return ocean::launch_surface_bounds(v, tile, base + rec_floats, rec, ctx->stream); },
                      "surface_bounds"))
        return r;
    ctx->bounds_valid[tile] = !ctx->disp_exposed;
    return OCEAN_OK;
}

// What a kernel with the air skip takes as `bounds`: those records, or null where OCEAN_RAY_BOUNDS=0 turns the skip
// (and the bounds launches) off.
int air_skip_bounds(ocean_ctx* ctx, int tile, const float** bounds) {
    *bounds = nullptr;
    return ctx->opt.ray_bounds ? ensure_bounds(ctx, tile, bounds) : OCEAN_OK;
}

// Ray casts: rays float[count][8] -> records float[count][8]; the staged forms take at most OCEAN_RAY_MAX_RAYS.
// The kernel runs behind the bounds launches where the air skip is on and the tile's bounds are stale.
struct RayCast {
    ocean_ctx* ctx;
    int tile, iterations, steps, refine;
    const float* rays;
    int count;
    float* out;

    int check(Form form) const {
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        if (!rays || !out) return fail(OCEAN_E_INVALID_ARG, "null rays or output");
        if (count < 0) return fail(OCEAN_E_INVALID_ARG, "negative ray count");
        if (form != Form::Device && count > OCEAN_RAY_MAX_RAYS)
            return fail(OCEAN_E_INVALID_ARG, "ray count " + std::to_string(count) + " > OCEAN_RAY_MAX_RAYS");
        if (steps < 1 || steps > OCEAN_RAY_MAX_STEPS)
            return fail(OCEAN_E_INVALID_ARG, "steps = " + std::to_string(steps) + " outside [1, OCEAN_RAY_MAX_STEPS]");
        const uint64_t samples = (uint64_t)count * (uint64_t)steps;
        if (samples > (uint64_t)OCEAN_RAY_MAX_SAMPLES)
            return fail(OCEAN_E_INVALID_ARG, "count * steps = " + std::to_string(samples) + " > OCEAN_RAY_MAX_SAMPLES");
        if (int r = check_iterations(iterations)) return r;
        if (refine < 0 || refine > 32) return fail(OCEAN_E_INVALID_ARG, "refine must be in [0, 32]");
        return check_tile(ctx, tile);
    }
    StateRule state() const { return {"ocean_raycast", "ray cast on"}; }
    StagedInputs inputs() const { return {"rays", 1, {{rays, (size_t)count * 8 * 4}}}; }
    size_t out_bytes() const { return (size_t)count * 8 * 4; }
    const char* lacks() const { return count == 0 ? "rays" : nullptr; }
    int launch(const float* const* in, float* d_out) const {
        const float* bounds;
        if (int r = air_skip_bounds(ctx, tile, &bounds)) return r;
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_raycast(v, tile, iterations, steps, refine, bounds, in[0], count, d_out,
                                                      ctx->stream);
                     },
                     "raycast");
    }
};

// Whitecap emitters: no inputs; (capacity + 1) records of 32 B.  What does not need the context is checked
// first, the _device form's alignment with it, so that a host learns of a bad argument whatever its context
// is.  The three kernels run over the context's scratch, which the first call allocates.
struct Whitecaps {
    ocean_ctx* ctx;
    int tile;
    float lod, threshold, x0, z0, dx, dz;
    int nx, ny, capacity;
    float* out;
    size_t bytes;

    int check(Form form) const {
        if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
        if (!std::isfinite(lod) || lod < 0.0f) return fail(OCEAN_E_INVALID_ARG, "lod must be finite and >= 0");
        if (!std::isfinite(threshold)) return fail(OCEAN_E_INVALID_ARG, "threshold must be finite");
        if (int r = check_region(x0, z0, dx, dz, nx, ny)) return r;
        if (capacity < 1 || capacity > OCEAN_WHITECAP_MAX_RECORDS)
            return fail(OCEAN_E_INVALID_ARG, "capacity = " + std::to_string(capacity) + " outside [1, OCEAN_WHITECAP_MAX_RECORDS]");
        const size_t want = ((size_t)capacity + 1) * 32;
        if (bytes != want)
            return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != (capacity + 1) * 32 = " +
                                                 std::to_string(want));
        if (form == Form::Device)
            if (int r = check_aligned(state().entry, inputs(), out)) return r;
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        return check_tile(ctx, tile);
    }
    StateRule state() const { return {"ocean_whitecaps", "whitecaps of", Needs::Turb}; }
    StagedInputs inputs() const { return {nullptr, 0, {}}; }
    size_t out_bytes() const { return bytes; }
    const char* lacks() const { return nullptr; }
    int launch(const float* const*, float* d_out) const {
        if (int r = ctx->whitecap_dev.ensure(ocean::whitecap_scratch_bytes())) return r;
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_whitecaps(v, ctx->vel, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity,
                                                        ctx->whitecap_dev.ptr, d_out, ctx->stream);
                     },
                     "whitecaps");
    }
};

// Camera views: no staged inputs, the rays follow from the camera's fourteen numbers, which travel to the kernel by
// value with the material; float[height][width][8], [height][width] or [height][width][4] by mode.  As for the
// whitecaps, what does not need the context is checked first, the _device form's alignment with it.  The kernel
// runs behind the bounds launches exactly as the ray casts' does.
struct Camera {
    ocean_ctx* ctx;
    int tile, mode, iterations, steps, refine;
    const float* camera;
    const float* material;
    int width, height;
    float* out;
    size_t bytes;

    static constexpr int kSkyMode = OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT;
    static size_t pixel_bytes(int mode) { return mode == OCEAN_CAMERA_HITS ? 32 : mode == OCEAN_CAMERA_RANGE ? 4 : 16; }
    int check(Form form) const { return check_as(form, state().entry, inputs()); }
    // entry, in: the family's own name and inputs (the camera with bodies runs these tests too)
    int check_as(Form form, const char* entry, const StagedInputs& in) const {
        if (!camera || !out) return fail(OCEAN_E_INVALID_ARG, "null camera or output");
        if (mode == (OCEAN_CAMERA_HITS | OCEAN_CAMERA_SKY_LUT) || mode == (OCEAN_CAMERA_RANGE | OCEAN_CAMERA_SKY_LUT))
            return fail(OCEAN_E_INVALID_ARG, "camera mode: OCEAN_CAMERA_SKY_LUT combines with OCEAN_CAMERA_COLOR only");
        if (mode != OCEAN_CAMERA_HITS && mode != OCEAN_CAMERA_RANGE && mode != OCEAN_CAMERA_COLOR && mode != kSkyMode)
            return fail(OCEAN_E_INVALID_ARG, "unknown camera mode");
        if ((mode == OCEAN_CAMERA_COLOR || mode == kSkyMode) && !material)
            return fail(OCEAN_E_INVALID_ARG, "OCEAN_CAMERA_COLOR needs a material");
        if (int r = check_iterations(iterations)) return r;
        if (steps < 1 || steps > OCEAN_RAY_MAX_STEPS)
            return fail(OCEAN_E_INVALID_ARG, "steps = " + std::to_string(steps) + " outside [1, OCEAN_RAY_MAX_STEPS]");
        if (refine < 0 || refine > 32) return fail(OCEAN_E_INVALID_ARG, "refine must be in [0, 32]");
        for (int k = 0; k < OCEAN_CAMERA_FLOATS; ++k)
            if (!std::isfinite(camera[k])) return fail(OCEAN_E_INVALID_ARG, "camera[" + std::to_string(k) + "] is not finite");
        for (int k = 0; material && k < OCEAN_CAMERA_MATERIAL_FLOATS; ++k)
            if (!std::isfinite(material[k])) return fail(OCEAN_E_INVALID_ARG, "material[" + std::to_string(k) + "] is not finite");
        if (width < 1 || height < 1) return fail(OCEAN_E_INVALID_ARG, "width and height must be at least 1");
        const uint64_t pixels = (uint64_t)width * (uint64_t)height;
        if (pixels > (uint64_t)OCEAN_CAMERA_MAX_PIXELS)
            return fail(OCEAN_E_INVALID_ARG, "width * height = " + std::to_string(pixels) + " > OCEAN_CAMERA_MAX_PIXELS");
        if (pixels * (uint64_t)steps > (uint64_t)OCEAN_CAMERA_MAX_SAMPLES)
            return fail(OCEAN_E_INVALID_ARG, "width * height * steps = " + std::to_string(pixels * (uint64_t)steps) +
                                                 " > OCEAN_CAMERA_MAX_SAMPLES");
        const size_t want = (size_t)pixels * pixel_bytes(mode);
        if (bytes != want)
            return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != width * height * " +
                                                 std::to_string(pixel_bytes(mode)) + " = " + std::to_string(want));
        if (form == Form::Device)
            if (int r = check_aligned(entry, in, out)) return r;
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        if (int r = check_tile(ctx, tile)) return r;
        // the async form's result is written into a readback slot
        if (form == Form::Async && bytes > stage_slot_bytes(ctx))
            return fail(OCEAN_E_INVALID_ARG, std::string(entry) + "_async: " + std::to_string(bytes) +
                                                 " B exceed a readback slot of " + std::to_string(stage_slot_bytes(ctx)) + " B");
        return OCEAN_OK;
    }
    StateRule state() const { return {"ocean_camera", "camera view of", Needs::Nothing, mode == kSkyMode}; }
    StagedInputs inputs() const { return {nullptr, 0, {}}; }
    size_t out_bytes() const { return bytes; }
    const char* lacks() const { return nullptr; }
    int launch(const float* const*, float* d_out) const {
        const float* bounds;
        if (int r = air_skip_bounds(ctx, tile, &bounds)) return r;
        ocean::CameraRays cam;
        ocean::CameraMaterial mat = {};
        std::copy(camera, camera + OCEAN_CAMERA_FLOATS, cam.c);
        if (material) std::copy(material, material + OCEAN_CAMERA_MATERIAL_FLOATS, mat.m);
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         if (mode == kSkyMode)
                             return ocean::launch_camera_sky(v, tile, iterations, steps, refine, bounds, cam, mat,
                                                             ctx->atm.view(OCEAN_LUT_SKYVIEW), ctx->atm.params.p[26], width,
                                                             height, ctx->opt.camera_tile != 0, d_out, ctx->stream);
                         return ocean::launch_camera(v, tile, mode, iterations, steps, refine, bounds, cam, mat, width, height,
                                                     ctx->opt.camera_tile != 0, d_out, ctx->stream);
                     },
                     "camera");
    }
};

// Camera views with bodies: the camera, with the box's six and the paint's four floats by value beside its own and
// the body records as its one staged input, (count - 1) * stride + 10 floats (none when count is 0).  Its own arguments
// first, none of which needs the context, then everything the camera refuses.  The async form's records can outgrow
// both a slot's room behind the image and its pinned copy (2 MiB at the limits), so they go through the slot's own
// block pair, as the spray's inputs do.
struct CameraBodies : Camera {
    const float* box;
    const float* paint;
    const float* bodies;
    int stride, count;

    int check(Form form) const { return check_bodies_as(form, state().entry); }
    // entry: the family's own name (the camera of the scene runs these tests too)
    int check_bodies_as(Form form, const char* entry) const {
        if (!box) return fail(OCEAN_E_INVALID_ARG, "null box");
        if ((mode == OCEAN_CAMERA_COLOR || mode == kSkyMode) && !paint)
            return fail(OCEAN_E_INVALID_ARG, "the colour modes need a paint");
        for (int k = 0; k < 6; ++k)
            if (!std::isfinite(box[k])) return fail(OCEAN_E_INVALID_ARG, "box[" + std::to_string(k) + "] is not finite");
        for (int k = 0; paint && k < OCEAN_BODY_PAINT_FLOATS; ++k)
            if (!std::isfinite(paint[k])) return fail(OCEAN_E_INVALID_ARG, "paint[" + std::to_string(k) + "] is not finite");
        if (stride < 10 || stride > 64) return fail(OCEAN_E_INVALID_ARG, "stride = " + std::to_string(stride) + " outside [10, 64]");
        if (count < 0 || count > OCEAN_BODY_MAX_BODIES)
            return fail(OCEAN_E_INVALID_ARG, "body count " + std::to_string(count) + " outside [0, OCEAN_BODY_MAX_BODIES]");
        if (count > 0 && !bodies) return fail(OCEAN_E_INVALID_ARG, "null bodies with count > 0");
        return check_as(form, entry, inputs());
    }
    StateRule state() const { return {"ocean_camera_bodies", "camera view of", Needs::Nothing, mode == kSkyMode}; }
    StagedInputs inputs() const {
        const size_t floats = count > 0 ? ((size_t)count - 1) * stride + 10 : 0;
        return {"bodies", count > 0 ? 1 : 0, {{bodies, floats * 4}}, 0, true};
    }
    int launch(const float* const* in, float* d_out) const {
        const float* bounds;
        if (int r = air_skip_bounds(ctx, tile, &bounds)) return r;
        ocean::CameraRays cam;
        ocean::CameraMaterial mat = {};
        ocean::BodyBox bx;
        ocean::BodyPaint pt = {};
        std::copy(camera, camera + OCEAN_CAMERA_FLOATS, cam.c);
        if (material) std::copy(material, material + OCEAN_CAMERA_MATERIAL_FLOATS, mat.m);
        std::copy(box, box + 6, bx.b);
        if (paint) std::copy(paint, paint + OCEAN_BODY_PAINT_FLOATS, pt.p);
        const bool sky = mode == kSkyMode;
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_camera_bodies(v, tile, mode, iterations, steps, refine, bounds, cam, mat,
                                                            sky ? ctx->atm.view(OCEAN_LUT_SKYVIEW) : ocean::LutView{},
                                                            sky ? ctx->atm.params.p[26] : 0.0f, bx, pt,
                                                            count > 0 ? in[0] : nullptr, stride, count,
                                                            ctx->opt.camera_cull != 0, width, height, d_out, ctx->stream);
                     },
                     "camera_bodies");
    }
};
static_assert(((size_t)OCEAN_BODY_MAX_BODIES * 64) * sizeof(float) <= kSprayInputBytes,
              "a slot's own block pair holds every camera request's bodies");

// Camera views in which the water sees the bodies: the camera with bodies, with the six `optics` floats by value
// beside the rest.  Its own arguments first (the optics, and its own set of modes), then everything the camera with
// bodies refuses: OCEAN_CAMERA_LINKS is 16 B per pixel and needs a material, as OCEAN_CAMERA_COLOR does, so those
// tests run with that mode in its place, but without a paint's being required.
struct CameraScene : CameraBodies {
    const float* optics;

    int check(Form form) const {
        if (!optics) return fail(OCEAN_E_INVALID_ARG, "null optics");
        for (int k = 0; k < OCEAN_SCENE_OPTICS_FLOATS; ++k)
            if (!std::isfinite(optics[k])) return fail(OCEAN_E_INVALID_ARG, "optics[" + std::to_string(k) + "] is not finite");
        if (optics[5] < 0.0f) return fail(OCEAN_E_INVALID_ARG, "optics[5] (reach) is negative");
        if (mode == OCEAN_CAMERA_HITS || mode == OCEAN_CAMERA_RANGE)
            return fail(OCEAN_E_INVALID_ARG, "scene mode: OCEAN_CAMERA_HITS and OCEAN_CAMERA_RANGE are ocean_camera_bodies*'s");
        if (mode != OCEAN_CAMERA_COLOR && mode != kSkyMode && mode != OCEAN_CAMERA_LINKS)
            return fail(OCEAN_E_INVALID_ARG, "unknown scene mode");
        if (mode != OCEAN_CAMERA_LINKS) return check_bodies_as(form, state().entry);
        if (!material) return fail(OCEAN_E_INVALID_ARG, "OCEAN_CAMERA_LINKS needs a material");
        CameraBodies as = *this;
        as.mode = OCEAN_CAMERA_COLOR;
        if (!paint) {  // not required, and not read: any finite paint passes in its place
            static const float kNoPaint[OCEAN_BODY_PAINT_FLOATS] = {};
            as.paint = kNoPaint;
        }
        return as.check_bodies_as(form, state().entry);
    }
    StateRule state() const { return {"ocean_camera_scene", "camera view of", Needs::Nothing, mode == kSkyMode}; }
    int launch(const float* const* in, float* d_out) const {
        const float* bounds;
        if (int r = air_skip_bounds(ctx, tile, &bounds)) return r;
        ocean::CameraRays cam;
        ocean::CameraMaterial mat;
        ocean::BodyBox bx;
        ocean::BodyPaint pt = {};
        ocean::SceneOptics op;
        std::copy(camera, camera + OCEAN_CAMERA_FLOATS, cam.c);
        std::copy(material, material + OCEAN_CAMERA_MATERIAL_FLOATS, mat.m);
        std::copy(box, box + 6, bx.b);
        if (paint) std::copy(paint, paint + OCEAN_BODY_PAINT_FLOATS, pt.p);
        std::copy(optics, optics + OCEAN_SCENE_OPTICS_FLOATS, op.o);
        const bool sky = mode == kSkyMode;
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_camera_scene(v, tile, mode, iterations, steps, refine, bounds, cam, mat,
                                                           sky ? ctx->atm.view(OCEAN_LUT_SKYVIEW) : ocean::LutView{},
                                                           sky ? ctx->atm.params.p[26] : 0.0f, bx, pt, op,
                                                           count > 0 ? in[0] : nullptr, stride, count,
                                                           ctx->opt.camera_cull != 0, width, height, d_out, ctx->stream);
                     },
                     "camera_scene");
    }
};

// Spray particles: the pool, (capacity + 1) records of 32 B, and the emitter list or none -> the stepped pool, with
// the sixteen `spray` floats by value.  As for the whitecaps, what does not need the context is checked first, the
// _device form's alignment (16 B for all three pointers: the kernels load and store float4) with it.  The staged
// forms take OCEAN_SPRAY_MAX_STAGED particles, and the async form's inputs outgrow a slot (StageSlot).  The three
// kernels run over the context's scratch, which grows to the largest call, behind the bounds launches exactly as
// the ray casts' kernel does.
struct Spray {
    ocean_ctx* ctx;
    int tile, iterations, substeps;
    const float* spray;
    const float* pool;
    int capacity;
    const float* emitters;
    int emit_capacity;
    float* out;
    size_t bytes;

    int check(Form form) const {
        if (!spray || !pool || !out) return fail(OCEAN_E_INVALID_ARG, "null spray, pool or output");
        if (int r = check_iterations(iterations)) return r;
        if (substeps < 1 || substeps > OCEAN_SPRAY_MAX_SUBSTEPS)
            return fail(OCEAN_E_INVALID_ARG, "substeps = " + std::to_string(substeps) + " outside [1, OCEAN_SPRAY_MAX_SUBSTEPS]");
        for (int k = 0; k < OCEAN_SPRAY_FLOATS; ++k) {
            if (!std::isfinite(spray[k])) return fail(OCEAN_E_INVALID_ARG, "spray[" + std::to_string(k) + "] is not finite");
            if (k >= 9 && spray[k] != 0.0f)
                return fail(OCEAN_E_INVALID_ARG, "spray[" + std::to_string(k) + "] is reserved and must be 0");
        }
        const int limit = form == Form::Device ? OCEAN_SPRAY_MAX_PARTICLES : OCEAN_SPRAY_MAX_STAGED;
        if (capacity < 1 || capacity > limit)
            return fail(OCEAN_E_INVALID_ARG, "capacity = " + std::to_string(capacity) + " outside [1, " +
                                                 (form == Form::Device ? "OCEAN_SPRAY_MAX_PARTICLES]" : "OCEAN_SPRAY_MAX_STAGED]"));
        if (emitters ? emit_capacity < 1 || emit_capacity > OCEAN_WHITECAP_MAX_RECORDS : emit_capacity != 0)
            return fail(OCEAN_E_INVALID_ARG, "emit_capacity = " + std::to_string(emit_capacity) +
                                                 (emitters ? " outside [1, OCEAN_WHITECAP_MAX_RECORDS]" : " without emitters (must be 0)"));
        const uint64_t steps = ((uint64_t)capacity + (uint64_t)emit_capacity) * (uint64_t)substeps;
        if (steps > ((uint64_t)1 << 24))
            return fail(OCEAN_E_INVALID_ARG, "(capacity + emit_capacity) * substeps = " + std::to_string(steps) + " > 1 << 24");
        const size_t want = ((size_t)capacity + 1) * 32;
        if (bytes != want)
            return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != (capacity + 1) * 32 = " +
                                                 std::to_string(want));
        if (form == Form::Device && ((((uintptr_t)pool | (uintptr_t)emitters | (uintptr_t)out) & 15) != 0))
            return fail(OCEAN_E_INVALID_ARG, "ocean_spray_step_device: pool, emitters and out must be 16-byte aligned");
        if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
        return check_tile(ctx, tile);
    }
    StateRule state() const { return {"ocean_spray_step", "spray steps on"}; }
    StagedInputs inputs() const {
        return {"pool and emitters",
                emitters ? 2 : 1,
                {{pool, bytes}, {emitters, emitters ? ((size_t)emit_capacity + 1) * 32 : 0}},
                0,
                true};
    }
    size_t out_bytes() const { return bytes; }
    const char* lacks() const { return nullptr; }
    int launch(const float* const* in, float* d_out) const {
        if (int r = ctx->spray_dev.ensure(ocean::spray_scratch_bytes(capacity, emit_capacity))) return r;
        const float* bounds;
        if (int r = air_skip_bounds(ctx, tile, &bounds)) return r;
        ocean::SprayParams sp;
        std::copy(spray, spray + OCEAN_SPRAY_FLOATS, sp.p);
        const ocean::DevView v = ctx->view();
        return timed(ctx, 2,
                     [&] {
                         return ocean::launch_spray_step(v, tile, iterations, substeps, sp, bounds, in[0], capacity,
                                                         emitters ? in[1] : nullptr, emit_capacity, ctx->spray_dev.ptr, d_out,
                                                         ctx->stream);
                     },
                     "spray_step");
    }
};

}  // namespace

extern "C" {

int ocean_query_surface_device(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                               float* out) {
    return device_form(SurfaceQuery{ctx, tile, mode, iterations, points, count, out});
}

int ocean_query_surface(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                        float* out) {
    return host_form(SurfaceQuery{ctx, tile, mode, iterations, points, count, out});
}

int ocean_query_surface_async(ocean_ctx* ctx, int tile, int mode, int iterations, const float* points, int count,
                              float* dst, ocean_readback** out) {
    return async_form(SurfaceQuery{ctx, tile, mode, iterations, points, count, dst}, out, "out");
}

int ocean_query_velocity_device(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* out) {
    return device_form(VelocityQuery{{ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, out}});
}

int ocean_query_velocity(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* out) {
    return host_form(VelocityQuery{{ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, out}});
}

int ocean_query_velocity_async(ocean_ctx* ctx, int tile, int iterations, const float* points, int count, float* dst,
                               ocean_readback** req) {
    return async_form(VelocityQuery{{ctx, tile, OCEAN_QUERY_SURFACE, iterations, points, count, dst}}, req);
}

int ocean_surface_grid_device(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                              float dx, float dz, int nx, int ny, float* out, size_t bytes) {
    return device_form(SurfaceGrid{ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes});
}

int ocean_surface_grid(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx,
                       float dz, int nx, int ny, float* out, size_t bytes) {
    return host_form(SurfaceGrid{ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes});
}

int ocean_surface_grid_async(ocean_ctx* ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                             float dx, float dz, int nx, int ny, float* out, size_t bytes, ocean_readback** req) {
    return async_form(SurfaceGrid{ctx, tile, mode, iterations, lod, x0, z0, dx, dz, nx, ny, out, bytes}, req);
}

int ocean_body_buoyancy_device(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                               const float* bodies, int count, float* out) {
    return device_form(BodyBuoyancy{ctx, tile, mode, iterations, hull, probes, bodies, count, out});
}

int ocean_body_buoyancy(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                        const float* bodies, int count, float* out) {
    return host_form(BodyBuoyancy{ctx, tile, mode, iterations, hull, probes, bodies, count, out});
}

int ocean_body_buoyancy_async(ocean_ctx* ctx, int tile, int mode, int iterations, const float* hull, int probes,
                              const float* bodies, int count, float* out, ocean_readback** req) {
    return async_form(BodyBuoyancy{ctx, tile, mode, iterations, hull, probes, bodies, count, out}, req);
}

int ocean_body_dynamics_device(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                               const float* bodies, const float* motion, int count, float* out) {
    return device_form(BodyDynamics{{ctx, tile, mode, iterations, hull, probes, bodies, count, out}, law, motion});
}

int ocean_body_dynamics(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                        const float* bodies, const float* motion, int count, float* out) {
    return host_form(BodyDynamics{{ctx, tile, mode, iterations, hull, probes, bodies, count, out}, law, motion});
}

int ocean_body_dynamics_async(ocean_ctx* ctx, int tile, int mode, int iterations, int law, const float* hull, int probes,
                              const float* bodies, const float* motion, int count, float* out, ocean_readback** req) {
    return async_form(BodyDynamics{{ctx, tile, mode, iterations, hull, probes, bodies, count, out}, law, motion}, req);
}

int ocean_body_step_device(ocean_ctx* ctx, int tile, int mode, int iterations, int law, int substeps, const float* step,
                           const float* hull, int probes, const float* props, const float* state, int count, float* out) {
    return device_form(BodyStep{{ctx, tile, mode, iterations, hull, probes, state, count, out}, law, substeps, step, props});
}

int ocean_body_step(ocean_ctx* ctx, int tile, int mode, int iterations, int law, int substeps, const float* step,
                    const float* hull, int probes, const float* props, const float* state, int count, float* out) {
    return host_form(BodyStep{{ctx, tile, mode, iterations, hull, probes, state, count, out}, law, substeps, step, props});
}

int ocean_body_step_async(ocean_ctx* ctx, int tile, int mode, int iterations, int law, int substeps, const float* step,
                          const float* hull, int probes, const float* props, const float* state, int count, float* out,
                          ocean_readback** req) {
    return async_form(BodyStep{{ctx, tile, mode, iterations, hull, probes, state, count, out}, law, substeps, step, props},
                      req);
}

int ocean_body_hydrostatics_device(ocean_ctx* ctx, int tile, int iterations, const float* vertices, int nverts,
                                   const void* triangles, int ntris, const float* bodies, int count, float* out) {
    return device_form(BodyHydrostatics{ctx, tile, iterations, vertices, nverts, static_cast<const int*>(triangles), ntris,
                                        bodies, count, out});
}

int ocean_body_hydrostatics(ocean_ctx* ctx, int tile, int iterations, const float* vertices, int nverts,
                            const void* triangles, int ntris, const float* bodies, int count, float* out) {
    return host_form(BodyHydrostatics{ctx, tile, iterations, vertices, nverts, static_cast<const int*>(triangles), ntris,
                                      bodies, count, out});
}

int ocean_body_hydrostatics_async(ocean_ctx* ctx, int tile, int iterations, const float* vertices, int nverts,
                                  const void* triangles, int ntris, const float* bodies, int count, float* out,
                                  ocean_readback** req) {
    return async_form(BodyHydrostatics{ctx, tile, iterations, vertices, nverts, static_cast<const int*>(triangles), ntris,
                                       bodies, count, out},
                      req);
}

int ocean_raycast_device(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                         float* out) {
    return device_form(RayCast{ctx, tile, iterations, steps, refine, rays, count, out});
}

int ocean_raycast(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                  float* out) {
    return host_form(RayCast{ctx, tile, iterations, steps, refine, rays, count, out});
}

int ocean_raycast_async(ocean_ctx* ctx, int tile, int iterations, int steps, int refine, const float* rays, int count,
                        float* dst, ocean_readback** req) {
    return async_form(RayCast{ctx, tile, iterations, steps, refine, rays, count, dst}, req);
}

int ocean_whitecaps_device(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                           int nx, int ny, int capacity, float* out, size_t bytes) {
    return device_form(Whitecaps{ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes});
}

int ocean_whitecaps(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz, int nx,
                    int ny, int capacity, float* out, size_t bytes) {
    return host_form(Whitecaps{ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes});
}

int ocean_whitecaps_async(ocean_ctx* ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                          int nx, int ny, int capacity, float* out, size_t bytes, ocean_readback** req) {
    return async_form(Whitecaps{ctx, tile, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out, bytes}, req);
}

int ocean_camera_device(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                        const float* material, int width, int height, float* out, size_t bytes) {
    return device_form(Camera{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes});
}

int ocean_camera(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                 const float* material, int width, int height, float* out, size_t bytes) {
    return host_form(Camera{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes});
}

int ocean_camera_async(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                       const float* material, int width, int height, float* out, size_t bytes, ocean_readback** req) {
    return async_form(Camera{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes}, req);
}

int ocean_camera_bodies_device(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                               const float* material, int width, int height, const float* box, const float* paint,
                               const float* bodies, int stride, int count, float* out, size_t bytes) {
    return device_form(CameraBodies{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                    box, paint, bodies, stride, count});
}

int ocean_camera_bodies(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                        const float* material, int width, int height, const float* box, const float* paint,
                        const float* bodies, int stride, int count, float* out, size_t bytes) {
    return host_form(CameraBodies{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                  box, paint, bodies, stride, count});
}

int ocean_camera_bodies_async(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                              const float* material, int width, int height, const float* box, const float* paint,
                              const float* bodies, int stride, int count, float* out, size_t bytes, ocean_readback** req) {
    return async_form(CameraBodies{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                   box, paint, bodies, stride, count},
                      req);
}

int ocean_camera_scene_device(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                              const float* material, int width, int height, const float* box, const float* paint,
                              const float* optics, const float* bodies, int stride, int count, float* out, size_t bytes) {
    return device_form(CameraScene{{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                    box, paint, bodies, stride, count},
                                   optics});
}

int ocean_camera_scene(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                       const float* material, int width, int height, const float* box, const float* paint,
                       const float* optics, const float* bodies, int stride, int count, float* out, size_t bytes) {
    return host_form(CameraScene{{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                  box, paint, bodies, stride, count},
                                 optics});
}

int ocean_camera_scene_async(ocean_ctx* ctx, int tile, int mode, int iterations, int steps, int refine, const float* camera,
                             const float* material, int width, int height, const float* box, const float* paint,
                             const float* optics, const float* bodies, int stride, int count, float* out, size_t bytes,
                             ocean_readback** req) {
    return async_form(CameraScene{{{ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out, bytes},
                                   box, paint, bodies, stride, count},
                                  optics},
                      req);
}

int ocean_spray_step_device(ocean_ctx* ctx, int tile, int iterations, int substeps, const float* spray, const float* pool,
                            int capacity, const float* emitters, int emit_capacity, float* out, size_t bytes) {
    return device_form(Spray{ctx, tile, iterations, substeps, spray, pool, capacity, emitters, emit_capacity, out, bytes});
}

int ocean_spray_step(ocean_ctx* ctx, int tile, int iterations, int substeps, const float* spray, const float* pool,
                     int capacity, const float* emitters, int emit_capacity, float* out, size_t bytes) {
    return host_form(Spray{ctx, tile, iterations, substeps, spray, pool, capacity, emitters, emit_capacity, out, bytes});
}

int ocean_spray_step_async(ocean_ctx* ctx, int tile, int iterations, int substeps, const float* spray, const float* pool,
                           int capacity, const float* emitters, int emit_capacity, float* out, size_t bytes,
                           ocean_readback** req) {
    return async_form(Spray{ctx, tile, iterations, substeps, spray, pool, capacity, emitters, emit_capacity, out, bytes},
                      req);
}

// World sampling has no async form and enters the device scope before its checks.
// (the caller has entered: OCEAN_ENTER)
static int check_sample(ocean_ctx* ctx, int tile, const float* pts, int count, float* out) {
    if (int r = check_tile(ctx, tile)) return r;
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
    if (int r = check_aligned("ocean_sample_world", {"points", 1, {{points, 0}}}, out)) return r;
    const ocean::DevView v = ctx->view();
    return timed(ctx, 2, [&] { return ocean::launch_sample_world(v, tile, points, count, out, ctx->stream); },
                 "sample_world");
}

int ocean_sample_world(ocean_ctx* ctx, int tile, const float* points, int count, float* out) {
    OCEAN_ENTER(ctx);
    if (int r = check_sample(ctx, tile, points, count, out)) return r;
    if (count == 0) return OCEAN_OK;
    return run_staged(ctx, "ocean_sample_world", {"points", 1, {{points, (size_t)count * 3 * 4}}}, out,
                      (size_t)count * 12 * 4, [&](const float* const* d_in, float* d_out) {
                          return ocean_sample_world_device(ctx, tile, d_in[0], count, d_out);
                      });
}

// The surface bounds stage nothing: the records are copied out of the context's own.
static int check_bounds(ocean_ctx* ctx, int tile, const float* out, size_t bytes) {
    if (!ctx) return fail(OCEAN_E_INVALID_ARG, "null context");
    if (!out) return fail(OCEAN_E_INVALID_ARG, "null output");
    if (int r = check_tile(ctx, tile)) return r;
    if (bytes != (size_t)ctx->C * 32)
        return fail(OCEAN_E_INVALID_ARG, "byte count " + std::to_string(bytes) + " != cascades * 32 = " +
                                             std::to_string((size_t)ctx->C * 32));
    return OCEAN_OK;
}

static const StateRule kBoundsState{"ocean_surface_bounds", "surface bounds of"};

int ocean_surface_bounds_device(ocean_ctx* ctx, int tile, float* out, size_t bytes) {
    if (int r = check_bounds(ctx, tile, out, bytes)) return r;
    if (int r = check_aligned(kBoundsState.entry, {nullptr, 0, {}}, out)) return r;
    if (int r = check_state(ctx, kBoundsState)) return r;
    OCEAN_ENTER(ctx);
    const float* rec = nullptr;
    if (int r = ensure_bounds(ctx, tile, &rec)) return r;
    OCEAN_HIP(hipMemcpyAsync(out, rec, bytes, hipMemcpyDeviceToDevice, ctx->stream));
    return OCEAN_OK;
}

int ocean_surface_bounds(ocean_ctx* ctx, int tile, float* out, size_t bytes) {
    if (int r = check_bounds(ctx, tile, out, bytes)) return r;
    if (int r = check_state(ctx, kBoundsState)) return r;
    OCEAN_ENTER(ctx);
    const float* rec = nullptr;
    if (int r = ensure_bounds(ctx, tile, &rec)) return r;
    OCEAN_HIP(hipMemcpyAsync(out, rec, bytes, hipMemcpyDeviceToHost, ctx->stream));
    OCEAN_HIP(hipStreamSynchronize(ctx->stream));
    return OCEAN_OK;
}

}  // extern "C"
