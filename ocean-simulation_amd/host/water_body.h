// WaterBody-shaped C++ host over the C ABI (include/ocean/ocean.h): the lifecycle of
// Assets/Scripts/Water/WaterBody.cs -- Awake (:211-256), the commented OnValidate
// re-init (:324-337), Update with an AsyncGPUReadback request EVERY frame (:284-297),
// GetWaterHeight (:195-209), OnDisable (:300-309) -- written the way a non-Python host
// binds the library.  It mirrors csharp/WaterBodyNative.cs call for call (the C# host
// cannot be compiled in this image: no dotnet), and abi_host.cpp drives it in a -m gpu
// test.  Header-only; errors throw std::runtime_error with ocean_last_error().
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <deque>
#include <stdexcept>
#include <string>
#include <vector>

#include "ocean/ocean.h"

namespace ocean_host {

inline void check(int rc, const char* where) {
    if (rc != OCEAN_OK) throw std::runtime_error(std::string(where) + " failed (" + std::to_string(rc) + "): " +
                                                 ocean_last_error());
}

// What Update reads back every frame: the height channel GetWaterHeight reads (ocean_read_height_async,
// 4 B per texel; the reference's buoyancyData is private, WaterBody.cs:58, and .g is all its reader uses)
// or the whole RGBA displacement slice (ocean_read_async, 16 B per texel) as the reference requests it.
// Probes reads no slice back: Update issues one ocean_query_surface_async per frame for the world positions
// given to SetProbes (one per buoyant body) and ProbeHeights is the newest landed answer, 32 B per probe over
// the link.  In that mode GetWaterHeight keeps returning 0, as the reference does before its first readback,
// and buoyancyData stays empty.
enum class Readback { Height, Rgba, Probes };

struct WaterCascade {  // WaterCascade.cs:10-24 (script defaults)
    float wavelength = 10.0f, cutoffHigh = 5.0f, cutoffLow = 0.0001f, swell = 0.4f, fade = 0.1f;
};

class WaterBody {
public:
    // WaterBody.cs:10-14, :29 (script defaults)
    float windSpeed = 1.0f, windDirectionX = 1.0f, windDirectionY = 1.0f;
    float gravity = 9.81f, fetch = 1.0f, depth = 4.0f;
    int texturesSize = 256;
    std::vector<WaterCascade> cascades{WaterCascade{}};
    uint64_t seed = 20251121;  // the reference's UnityEngine.Random is unseeded; this library's generator is
    int device = 0;
    size_t maxReadbacksInFlight = 4;  // bound on queued requests (set before Awake): 2-4 keep the copies back to
                                      // back beside the frames; 8 stretch each
    Readback readback = Readback::Height;  // set before Awake
    int probeMode = OCEAN_QUERY_SURFACE;   // Readback::Probes: ocean_query_surface_async's mode ...
    int probeIterations = 4;               // ... and fixed-point steps (0 with OCEAN_QUERY_REFERENCE)
    bool velocity = false;      // set before Awake: also keep the VELOCITY texture (Velocity)
    size_t probeCapacity = 64;  // probes the pinned ring is sized for at Awake (or the probes set by then, if more)

    WaterBody() = default;
    WaterBody(const WaterBody&) = delete;
    WaterBody& operator=(const WaterBody&) = delete;
    ~WaterBody() { OnDisable(); }

    void Awake() {
        check(ocean_create(device, texturesSize, (int)cascades.size(), 1, OCEAN_F_MIPS | (velocity ? OCEAN_F_VELOCITY : 0u),
                           &ctx_),
              "ocean_create");
        ApplyParams();
        check(ocean_generate_noise(ctx_, seed), "ocean_generate_noise");
        check(ocean_init_spectrum(ctx_), "ocean_init_spectrum");
        probe_cap_ = std::max<size_t>({probeCapacity, probes_.size() / 2, 1});
        if (readback == Readback::Probes && probe_cap_ > OCEAN_QUERY_MAX_POINTS)
            throw std::runtime_error("at most OCEAN_QUERY_MAX_POINTS probes");
        // the readback ring: maxReadbacksInFlight pinned slices, plus the one the last landed slice stays
        // in, allocated once and reused, freed only in OnDisable (hipHostFree synchronizes the device,
        // so a free per request would make every Update wait for the frame it just queued)
        for (size_t i = 0; i < std::max<size_t>(maxReadbacksInFlight, 1) + 1; ++i) {
            void* b = nullptr;
            check(ocean_host_alloc(SliceBytes(), &b), "ocean_host_alloc");
            free_.push_back(b);
            owned_.push_back(b);
        }
    }

    // Parameter change -> spectrum re-init; the foam accumulator carries over, as there.
    void OnValidate() {
        if (!ctx_) return;
        ApplyParams();
        check(ocean_init_spectrum(ctx_), "ocean_init_spectrum");
    }

    void CalculateWavesTexturesAtTime(float time) { check(ocean_step(ctx_, time), "ocean_step"); }

    // Step, then request the displacement slice 0; requests complete in order and each
    // completed one refreshes buoyancyData (the reference's callback, :292-295).
    void Update(float time) {
        CalculateWavesTexturesAtTime(time);
        while (!readbacks_.empty()) {
            const int st = ocean_readback_status(readbacks_.front().req);
            if (st == 0) break;
            Complete(st);
        }
        if (readback == Readback::Probes && probes_.empty()) return;  // nobody asks: no request
        // at most maxReadbacksInFlight requests queued (the ring's extra slot holds the landed slice):
        // when full, wait for the oldest
        while (!readbacks_.empty() && (readbacks_.size() >= std::max<size_t>(maxReadbacksInFlight, 1) || free_.empty())) {
            const int st = ocean_readback_wait(readbacks_.front().req) == OCEAN_OK ? 1 : -1;
            Complete(st);
        }
        Pending p;
        p.buf = free_.back();
        free_.pop_back();
        p.count = probes_.size() / 2;
        // Probes: one query for every probe, in place of the slice request: 32 B per probe come back
        const int rc = readback == Readback::Probes
                           ? ocean_query_surface_async(ctx_, 0, probeMode, probeIterations, probes_.data(), (int)p.count,
                                                       static_cast<float*>(p.buf), &p.req)
                       : readback == Readback::Height
                           ? ocean_read_height_async(ctx_, 0, 0, static_cast<float*>(p.buf), SliceBytes(), &p.req)
                           : ocean_read_async(ctx_, OCEAN_TEX_DISP, 0, 0, p.buf, SliceBytes(), &p.req);
        if (rc != OCEAN_OK) {
            free_.push_back(p.buf);
            check(rc, readback == Readback::Probes   ? "ocean_query_surface_async"
                      : readback == Readback::Height ? "ocean_read_height_async"
                                                     : "ocean_read_async");
        }
        readbacks_.push_back(p);
        ++requested_;
    }

    void WaitForReadbacks() {
        while (!readbacks_.empty()) {
            const int st = ocean_readback_wait(readbacks_.front().req) == OCEAN_OK ? 1 : -1;
            Complete(st);
        }
    }

    // WaterBody.cs:195-209, with its mapping of world x, z over [-texturesSize/2, texturesSize/2].
    float GetWaterHeight(float worldX, float worldZ) const {
        if (!held_ || readback == Readback::Probes) return 0.0f;
        auto inverse_lerp = [](float a, float b, float v) {
            return a == b ? 0.0f : std::min(std::max((v - a) / (b - a), 0.0f), 1.0f);
        };
        const int n = texturesSize;
        const float u = inverse_lerp((float)(-n / 2), (float)(n / 2), worldX);
        const float v = inverse_lerp((float)(-n / 2), (float)(n / 2), worldZ);
        const int x = std::min(std::max((int)(u * n), 0), n - 1);
        const int y = std::min(std::max((int)(v * n), 0), n - 1);
        const size_t t = (size_t)y * n + x;
        return readback == Readback::Height ? held_[t] : held_[t * 4 + 1];  // .g = Dy
    }

    // The world positions Update asks about with Readback::Probes: [M][3] (x, y, z; x and z are used, as
    // GetWaterHeight uses its worldPosition).  After Awake, at most the capacity the ring was sized for.
    // Takes effect at the next Update; answers already in flight keep their own M.
    void SetProbes(const std::vector<float>& xyz) {
        if (ctx_ && readback == Readback::Probes && xyz.size() / 3 > probe_cap_)
            throw std::runtime_error("more probes than the capacity the ring was sized for at Awake");
        probes_.clear();
        for (size_t i = 0; i + 2 < xyz.size(); i += 3) {
            probes_.push_back(xyz[i]);
            probes_.push_back(xyz[i + 2]);
        }
    }

    // The newest landed query, [M][8] as ocean_query_surface returns it, or empty before the first lands.
    std::vector<float> ProbeResults() const {
        if (readback != Readback::Probes || !held_) return {};
        return std::vector<float>(held_, held_ + held_count_ * 8);
    }

    // The newest landed heights, [M] in SetProbes' order, or empty before the first lands.
    std::vector<float> ProbeHeights() const {
        std::vector<float> h;
        if (readback != Readback::Probes || !held_) return h;
        for (size_t i = 0; i < held_count_; ++i) h.push_back(held_[i * 8]);
        return h;
    }

    // What Water.shader reads at world positions (x, z, lod) -> 12 floats per point.
    std::vector<float> SampleWorld(const std::vector<float>& points) const {
        std::vector<float> out(points.size() / 3 * 12);
        check(ocean_sample_world(ctx_, 0, points.data(), (int)(points.size() / 3), out.data()), "ocean_sample_world");
        return out;
    }

    // The surface over a regular grid (ocean.h ocean_surface_grid): node (i, j) at (x0 + i dx, z0 + j dz) is element
    // j * nx + i of the result.  OCEAN_GRID_VERTICES (iterations 0, `lod` as SampleWorld): 8 floats per node, the
    // displaced vertex x, y, z, the foam, the normal, 0: MeshGenerator's plane through the domain stage of
    // Water.shader; OCEAN_GRID_SURFACE: ocean_query_surface's record at every node; OCEAN_GRID_HEIGHTFIELD: its
    // height alone, 1 float per node.  The per-frame call of a renderer or a heightfield collider.
    std::vector<float> SurfaceGrid(float x0, float z0, float dx, float dz, int nx, int ny, int mode = OCEAN_GRID_SURFACE,
                                   int iterations = 4, float lod = 0.0f) const {
        const size_t per = mode == OCEAN_GRID_HEIGHTFIELD ? 1 : 8;
        // (a size outside the limits is refused by the library; no buffer of that size first)
        const bool valid = nx >= 1 && ny >= 1 && (long long)nx * ny <= OCEAN_GRID_MAX_NODES;
        std::vector<float> out(valid ? (size_t)nx * ny * per : 0);
        check(ocean_surface_grid(ctx_, 0, mode, mode == OCEAN_GRID_VERTICES ? 0 : iterations, lod, x0, z0, dx, dz, nx, ny,
                                 out.data(), out.size() * sizeof(float)),
              "ocean_surface_grid");
        return out;
    }

    // BuoyantObject.FixedUpdate's lookup for M bodies of P probes each (ocean.h ocean_body_buoyancy): hull is
    // [P][5] = (cell centre in the body frame, vertical extent, volume), bodies [M][10] = (origin, body -> world
    // quaternion xyzw, per-axis scale) -> 8 floats per body: submerged volume V, V * centroid relative to the
    // origin, V-weighted water normal, worst residual.  Force rho g V along +y; torque rho g (-out[3], 0, out[1]).
    std::vector<float> Buoyancy(const std::vector<float>& hull, const std::vector<float>& bodies, int iterations = 4,
                                int mode = OCEAN_QUERY_SURFACE) const {
        std::vector<float> out(bodies.size() / 10 * 8);
        check(ocean_body_buoyancy(ctx_, 0, mode, iterations, hull.data(), (int)(hull.size() / 5), bodies.data(),
                                  (int)(bodies.size() / 10), out.data()),
              "ocean_body_buoyancy");
        return out;
    }

    // The hydrostatic pressure over the wetted triangles of a mesh shared by M bodies (ocean.h ocean_body_hydrostatics):
    // vertices [V][3] in the body frame, triangles [T][3] wound counter-clockwise seen from outside, bodies [M][10] as
    // Buoyancy takes them -> 16 floats per body: sum F, wetted area, sum Tq about the origin, worst residual, the wetted
    // area's first moment, wet triangles, draught, wet vertices, sum Av.y, 0.  Force rho g out[0..2], torque
    // rho g out[4..6], heave stiffness rho g (-out[14]).  The reference has no counterpart.
    std::vector<float> Hydrostatics(const std::vector<float>& vertices, const std::vector<int>& triangles,
                                    const std::vector<float>& bodies, int iterations = 4) const {
        std::vector<float> out(bodies.size() / 10 * OCEAN_HULL_RECORD_FLOATS);
        check(ocean_body_hydrostatics(ctx_, 0, iterations, vertices.data(), (int)(vertices.size() / 3), triangles.data(),
                                      (int)(triangles.size() / 3), bodies.data(), (int)(bodies.size() / 10), out.data()),
              "ocean_body_hydrostatics");
        return out;
    }

    // Buoyancy's records with the drag against the water's own velocity beside them (ocean.h ocean_body_dynamics;
    // `velocity` set before Awake): motion [M][6] = (world linear velocity of the body origin, world angular
    // velocity) -> 16 floats per body: Buoyancy's 8, then sum F, sum T about the origin, the largest relative speed
    // over the wet probes and their number.  Drag force k out[8..10], torque k out[11..13] for the host's k.
    std::vector<float> Dynamics(const std::vector<float>& hull, const std::vector<float>& bodies,
                                const std::vector<float>& motion, int iterations = 4, int mode = OCEAN_QUERY_SURFACE,
                                int law = OCEAN_DRAG_LINEAR) const {
        if (motion.size() / 6 != bodies.size() / 10) throw std::runtime_error("Dynamics: one motion per body");
        std::vector<float> out(bodies.size() / 10 * 16);
        check(ocean_body_dynamics(ctx_, 0, mode, iterations, law, hull.data(), (int)(hull.size() / 5), bodies.data(),
                                  motion.data(), (int)(bodies.size() / 10), out.data()),
              "ocean_body_dynamics");
        return out;
    }

    // BuoyantObject.FixedUpdate for M bodies of P probes each, `substeps` fixed updates against this frame's water in
    // one launch (ocean.h ocean_body_step; `velocity` set before Awake): state [M][32] = (bodies' 10, motion's 6, 16
    // ignored), props [M][4] = (1 / mass, 1 / Ix, 1 / Iy, 1 / Iz), step [8] = (h, g, B, kd, kt, la, aa, 0) -> 32 floats
    // per body: the state after the last substep, then Dynamics' record of that substep; the result is the next
    // call's state.  async: through ocean_body_step_async and a pinned buffer, waited for here (what a host that
    // overlaps the copy with its frame does, in one place).
    std::vector<float> StepBodies(const std::vector<float>& hull, const std::vector<float>& state,
                                  const std::vector<float>& props, const std::vector<float>& step, int substeps = 1,
                                  int iterations = 4, int mode = OCEAN_QUERY_SURFACE, int law = OCEAN_DRAG_LINEAR,
                                  bool async = false) const {
        const int count = (int)(state.size() / 32);
        if (props.size() / 4 != state.size() / 32) throw std::runtime_error("StepBodies: one props record per body");
        if (step.size() != OCEAN_BODY_STEP_FLOATS) throw std::runtime_error("StepBodies: step is float[8]");
        std::vector<float> out(state.size() / 32 * 32);
        if (!async) {
            check(ocean_body_step(ctx_, 0, mode, iterations, law, substeps, step.data(), hull.data(), (int)(hull.size() / 5),
                                  props.data(), state.data(), count, out.data()),
                  "ocean_body_step");
            return out;
        }
        void* pinned = nullptr;
        check(ocean_host_alloc(out.size() * sizeof(float), &pinned), "ocean_host_alloc");
        ocean_readback* req = nullptr;
        int rc = ocean_body_step_async(ctx_, 0, mode, iterations, law, substeps, step.data(), hull.data(),
                                       (int)(hull.size() / 5), props.data(), state.data(), count, static_cast<float*>(pinned),
                                       &req);
        if (rc == OCEAN_OK) {
            rc = ocean_readback_wait(req);
            if (rc == OCEAN_OK) std::copy(static_cast<float*>(pinned), static_cast<float*>(pinned) + out.size(), out.begin());
            ocean_readback_release(req);
        }
        ocean_host_free(pinned);
        check(rc, "ocean_body_step_async");
        return out;
    }

    // The water's velocity at M world positions (ocean.h ocean_query_velocity; `velocity` set before Awake):
    // points [M][2] = (world x, world z) -> 8 floats per point: velocity x, y, z of the water particle on the
    // surface above the point, residual, height, p.x, p.z, dDxz/dt.  What drag relative to the water and particle
    // advection need; the reference's BuoyantObject drags against still water.
    std::vector<float> Velocity(const std::vector<float>& points, int iterations = 4) const {
        std::vector<float> out(points.size() / 2 * 8);
        check(ocean_query_velocity(ctx_, 0, iterations, points.data(), (int)(points.size() / 2), out.data()),
              "ocean_query_velocity");
        return out;
    }

    // Ray casts against the surface (ocean.h ocean_raycast): rays [M][8] = (origin x, y, z, direction x, y, z, t0,
    // t1) -> 8 floats per ray: t*, the ray point's height over the water there, the fixed point's residual, the
    // status (OCEAN_RAY_MISS / _HIT / _SUBMERGED), the normal and the foam at the point met, origin + t* direction.
    // The water's Physics.Raycast; the reference has none.
    std::vector<float> Raycast(const std::vector<float>& rays, int iterations = 4, int steps = 64, int refine = 8) const {
        std::vector<float> out(rays.size() / 8 * 8);
        check(ocean_raycast(ctx_, 0, iterations, steps, refine, rays.data(), (int)(rays.size() / 8), out.data()),
              "ocean_raycast");
        return out;
    }

    // What a camera sees of the water (ocean.h ocean_camera): camera = 14 floats (eye, the direction through pixel
    // (0, 0), its change per column and per row, t0, t1); pixel (i, j) is element j * width + i of the result.
    // OCEAN_CAMERA_COLOR shades the fragment stage of Water.shader with the 32 floats of `material`: r, g, b, status
    // per pixel; OCEAN_CAMERA_RANGE: the distance along each ray, +infinity where it misses; OCEAN_CAMERA_HITS:
    // Raycast's 8 floats per pixel (both with an empty material).  The headless stand-in for the reference's renderer.
    std::vector<float> Camera(const std::vector<float>& camera, int width, int height, int mode = OCEAN_CAMERA_COLOR,
                              const std::vector<float>& material = {}, int iterations = 4, int steps = 64,
                              int refine = 8) const {
        if (camera.size() != OCEAN_CAMERA_FLOATS || (!material.empty() && material.size() != OCEAN_CAMERA_MATERIAL_FLOATS))
            throw std::runtime_error("Camera: camera is 14 floats, material 32 or none");
        const size_t per = mode == OCEAN_CAMERA_HITS ? 8 : mode == OCEAN_CAMERA_RANGE ? 1 : 4;
        // (a size outside the limits is refused by the library; no buffer of that size first)
        const bool valid = width >= 1 && height >= 1 && (long long)width * height <= OCEAN_CAMERA_MAX_PIXELS;
        std::vector<float> out(valid ? (size_t)width * height * per : 0);
        check(ocean_camera(ctx_, 0, mode, iterations, steps, refine, camera.data(), material.empty() ? nullptr : material.data(),
                           width, height, out.data(), out.size() * sizeof(float)),
              "ocean_camera");
        return out;
    }

    // Camera with the boxes of `bodies` in the picture (ocean.h ocean_camera_bodies): `bodies` holds records `stride`
    // floats apart whose first ten floats are (c, q, s), the `bodies` of Buoyancy (stride 10) or the records StepBodies
    // returns (stride 32); `box` = 6 floats (lo, hi) of the one box they share, `paint` = 4 floats (r, g, b, ka), empty
    // outside the colour modes.  A body pixel has the status OCEAN_RAY_BODY; OCEAN_CAMERA_HITS carries its distance,
    // its normal and the body's index.
    std::vector<float> CameraBodies(const std::vector<float>& camera, int width, int height, const std::vector<float>& box,
                                    const std::vector<float>& paint, const std::vector<float>& bodies, int stride = 10,
                                    int mode = OCEAN_CAMERA_COLOR, const std::vector<float>& material = {},
                                    int iterations = 4, int steps = 64, int refine = 8) const {
        if (camera.size() != OCEAN_CAMERA_FLOATS || (!material.empty() && material.size() != OCEAN_CAMERA_MATERIAL_FLOATS))
            throw std::runtime_error("CameraBodies: camera is 14 floats, material 32 or none");
        if (box.size() != 6 || (!paint.empty() && paint.size() != OCEAN_BODY_PAINT_FLOATS) || stride < 10)
            throw std::runtime_error("CameraBodies: box is 6 floats, paint 4 or none, stride at least 10");
        const size_t per = mode == OCEAN_CAMERA_HITS ? 8 : mode == OCEAN_CAMERA_RANGE ? 1 : 4;
        const bool valid = width >= 1 && height >= 1 && (long long)width * height <= OCEAN_CAMERA_MAX_PIXELS;
        std::vector<float> out(valid ? (size_t)width * height * per : 0);
        const int count = bodies.empty() ? 0 : (int)((bodies.size() + (size_t)stride - 10) / (size_t)stride);
        check(ocean_camera_bodies(ctx_, 0, mode, iterations, steps, refine, camera.data(),
                                  material.empty() ? nullptr : material.data(), width, height, box.data(),
                                  paint.empty() ? nullptr : paint.data(), bodies.empty() ? nullptr : bodies.data(), stride,
                                  count, out.data(), out.size() * sizeof(float)),
              "ocean_camera_bodies");
        return out;
    }

    // CameraBodies with the water seeing the bodies (ocean.h ocean_camera_scene): their shadows on it, their reflections
    // in it and their submerged parts through it.  `optics` = 6 floats (shadow colour r, g, b, shadow intensity, water
    // fog density, reach of the secondary rays in metres); mode OCEAN_CAMERA_COLOR, OCEAN_CAMERA_COLOR |
    // OCEAN_CAMERA_SKY_LUT or OCEAN_CAMERA_LINKS (per pixel: lit or not, the body seen through the water, the body
    // reflected, the status), 4 floats per pixel in each; the material is required, the paint in the colour modes.
    std::vector<float> CameraScene(const std::vector<float>& camera, int width, int height, const std::vector<float>& box,
                                   const std::vector<float>& paint, const std::vector<float>& optics,
                                   const std::vector<float>& bodies, int stride, int mode, const std::vector<float>& material,
                                   int iterations = 4, int steps = 64, int refine = 8) const {
        if (camera.size() != OCEAN_CAMERA_FLOATS || material.size() != OCEAN_CAMERA_MATERIAL_FLOATS)
            throw std::runtime_error("CameraScene: camera is 14 floats, material 32");
        if (box.size() != 6 || (!paint.empty() && paint.size() != OCEAN_BODY_PAINT_FLOATS) ||
            optics.size() != OCEAN_SCENE_OPTICS_FLOATS || stride < 10)
            throw std::runtime_error("CameraScene: box is 6 floats, paint 4 or none, optics 6, stride at least 10");
        const bool valid = width >= 1 && height >= 1 && (long long)width * height <= OCEAN_CAMERA_MAX_PIXELS;
        std::vector<float> out(valid ? (size_t)width * height * 4 : 0);
        const int count = bodies.empty() ? 0 : (int)((bodies.size() + (size_t)stride - 10) / (size_t)stride);
        check(ocean_camera_scene(ctx_, 0, mode, iterations, steps, refine, camera.data(), material.data(), width, height,
                                 box.data(), paint.empty() ? nullptr : paint.data(), optics.data(),
                                 bodies.empty() ? nullptr : bodies.data(), stride, count, out.data(),
                                 out.size() * sizeof(float)),
              "ocean_camera_scene");
        return out;
    }

    // The atmosphere of AtmosphereController.cs (ocean.h "The atmosphere"): its Awake, the transmittance and the
    // multiscatter table from the 32 floats of `params` (ocean.h names them; DefaultAtmosphere() has the reference's),
    // at the reference's sizes when `dims` is empty, else (Tw, Th, Mw, Mh, Sw, Sh).  Needs no spectrum.
    static std::vector<float> DefaultAtmosphere() {
        return {6360000.0f, 6420000.0f, 5.802e-6f, 13.558e-6f, 6.5e-5f, 0.0f,  0.0f,  0.0f,      8000.0f,   3.996e-6f, 3.996e-6f,
                3.996e-6f,  4.4e-6f,    4.4e-6f,   4.4e-6f,    1200.0f, 0.85f, 0.0f,  0.0f,      0.0f,      0.65e-6f,  1.881e-6f,
                0.085e-6f,  0.0f,       0.0f,      0.0f,       0.04f,   0.0f,  0.0f,  0.0f,      0.0f,      0.0f};
    }
    void Atmosphere(const std::vector<float>& params = DefaultAtmosphere(), const std::vector<int>& dims = {}) const {
        if (params.size() != OCEAN_ATMOSPHERE_FLOATS || (!dims.empty() && dims.size() != 6))
            throw std::runtime_error("Atmosphere: params is 32 floats, dims six sizes or none");
        const int zero[6] = {0, 0, 0, 0, 0, 0};
        const int* d = dims.empty() ? zero : dims.data();
        check(ocean_atmosphere(ctx_, params.data(), d[0], d[1], d[2], d[3], d[4], d[5]), "ocean_atmosphere");
    }

    // AtmosphereController.Update: the sky-view table for the direction towards the sun (any length), and the colour
    // of its light, which goes into a camera material's [23..25].  Camera(..., OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT)
    // then reflects that sky.
    std::vector<float> SkyUpdate(const std::vector<float>& sun) const {
        if (sun.size() != 3) throw std::runtime_error("SkyUpdate: sun is 3 floats");
        check(ocean_sky_update(ctx_, sun.data()), "ocean_sky_update");
        std::vector<float> rgb(3);
        check(ocean_sun_color(ctx_, sun.data(), rgb.data()), "ocean_sun_color");
        return rgb;
    }

    // One of the atmosphere's tables (OCEAN_LUT_*): float4 [height][width].
    std::vector<float> AtmosphereLut(int which, int* width, int* height) const {
        void* dev = nullptr;
        size_t w = 0, h = 0;
        check(ocean_atmosphere_lut(ctx_, which, &dev, &w, &h), "ocean_atmosphere_lut");
        std::vector<float> out(w * h * 4);
        check(ocean_atmosphere_read(ctx_, which, out.data(), out.size() * sizeof(float)), "ocean_atmosphere_read");
        *width = (int)w;
        *height = (int)h;
        return out;
    }

    // Where the sea is breaking (ocean.h ocean_whitecaps): the nodes (i, j) at (x0 + i dx, z0 + j dz) whose foam
    // reaches `threshold`, in ascending j * nx + i.  Returns the list as the library writes it, capacity + 1 records
    // of 8 floats: the header (eight uint32: T selected, W = min(T, capacity) written, nx * ny, capacity, 0, 0, 0, 0;
    // WhitecapHeader reads it), then W records: displaced x, y, z, foam, the water's velocity x, y, z (`velocity` set
    // before Awake, else 0), (float)(j * nx + i); the records past W are zero.  Spawn points for spray and foam
    // particles; the reference has the foam only as a shading term (Water.shader:343).
    std::vector<float> Whitecaps(float threshold, float x0, float z0, float dx, float dz, int nx, int ny, int capacity,
                                 float lod = 0.0f) const {
        std::vector<float> out(((size_t)std::max(capacity, 0) + 1) * 8);
        check(ocean_whitecaps(ctx_, 0, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, out.data(),
                              out.size() * sizeof(float)),
              "ocean_whitecaps");
        uint32_t head[8];
        WhitecapHeader(out, head);
        std::fill(out.begin() + 8 * ((size_t)head[1] + 1), out.end(), 0.0f);  // unspecified in the library's output
        return out;
    }

    // The eight uint32 of a whitecap list's header (its floats hold their bits).
    static void WhitecapHeader(const std::vector<float>& list, uint32_t head[8]) {
        std::memcpy(head, list.data(), 8 * sizeof(uint32_t));
    }

    // Spray particles (ocean.h ocean_spray_step): `pool` holds capacity + 1 records of 8 floats, the header and the
    // particles (position, age, velocity, tag); one fresh particle is spawned per record of the whitecap list `emitters`
    // (as Whitecaps returns it, or empty for none); all take `substeps` substeps under the 16 floats of `spray` (h, g,
    // kd, wind x, y, z, life, jet, lift, zeros) against this frame's water, and those that fall back into the sea or
    // outlive their life are retired.  Returns the stepped pool, the records past W zero: the next call's `pool`.
    // EmptyPool(capacity) starts one.  The reference has no particles.
    std::vector<float> Spray(const std::vector<float>& spray, const std::vector<float>& pool,
                             const std::vector<float>& emitters = {}, int substeps = 1, int iterations = 2) const {
        if (spray.size() != OCEAN_SPRAY_FLOATS || pool.size() < 8 || pool.size() % 8 || emitters.size() % 8)
            throw std::runtime_error("Spray: spray is 16 floats, pool and emitters records of 8");
        const int capacity = (int)(pool.size() / 8) - 1;
        const int emit_capacity = emitters.empty() ? 0 : (int)(emitters.size() / 8) - 1;
        std::vector<float> out(pool.size());
        check(ocean_spray_step(ctx_, 0, iterations, substeps, spray.data(), pool.data(), capacity,
                               emitters.empty() ? nullptr : emitters.data(), emit_capacity, out.data(),
                               out.size() * sizeof(float)),
              "ocean_spray_step");
        uint32_t head[8];
        WhitecapHeader(out, head);  // the same layout
        std::fill(out.begin() + 8 * ((size_t)head[1] + 1), out.end(), 0.0f);  // unspecified in the library's output
        return out;
    }
    static std::vector<float> EmptyPool(int capacity) { return std::vector<float>(((size_t)capacity + 1) * 8, 0.0f); }

    // The per-cascade bounds of the displacement (ocean.h ocean_surface_bounds): 8 floats per cascade, (min x, y,
    // z, w, max x, y, z, w); their cascade sums bound the displaced mesh.
    std::vector<float> SurfaceBounds() const {
        std::vector<float> out(cascades.size() * 8);
        check(ocean_surface_bounds(ctx_, 0, out.data(), out.size() * sizeof(float)), "ocean_surface_bounds");
        return out;
    }

    std::vector<float> ReadSlice(int texture, int cascade) const {
        std::vector<float> out(SliceBytes() / 4);
        check(ocean_read(ctx_, texture, 0, cascade, out.data(), SliceBytes()), "ocean_read");
        return out;
    }

    void OnDisable() {
        for (auto& p : readbacks_) ocean_readback_release(p.req);
        readbacks_.clear();
        if (held_slot_) {  // the last landed slice outlives the pinned ring
            last_.assign(held_, held_ + HeldFloats());
            held_ = last_.data();
            held_slot_ = nullptr;
        }
        for (void* b : owned_) ocean_host_free(b);
        owned_.clear();
        free_.clear();
        if (ctx_) ocean_destroy(ctx_);
        ctx_ = nullptr;
    }

    // The last landed displacement slice 0 (WaterBody.cs:295's array): [y][x] heights (Readback::Height)
    // or [y][x][rgba] (Readback::Rgba); empty before the first readback lands.  Copied out of its pinned slot once, on the first call after it lands; later
    // calls return the same array until the next readback lands (the reference reads a field).
    const std::vector<float>& buoyancyData() {
        if (held_ && !buoy_valid_ && readback != Readback::Probes) {
            buoy_.assign(held_, held_ + SliceBytes() / 4);
            buoy_valid_ = true;
        }
        if (!held_ || readback == Readback::Probes) buoy_.clear();
        return buoy_;
    }
    // The context itself, for a host that also calls entries this facade does not wrap (null outside Awake ..
    // OnDisable; the facade keeps owning it).
    ocean_ctx* Context() const { return ctx_; }
    long requested() const { return requested_; }
    long completed() const { return completed_; }

private:
    struct Pending {
        ocean_readback* req = nullptr;
        void* buf = nullptr;
        size_t count = 0;  // Probes: the points of this request
    };
    ocean_ctx* ctx_ = nullptr;
    std::deque<Pending> readbacks_;
    std::vector<void*> free_, owned_;  // pinned readback ring: idle slots, all slots
    const float* held_ = nullptr;  // the last landed slice, in its pinned slot (out of the ring)
    void* held_slot_ = nullptr;
    size_t held_count_ = 0;       // Probes: the points of the landed query
    std::vector<float> probes_;   // SetProbes' (world x, world z) pairs
    size_t probe_cap_ = 0;
    std::vector<float> last_;  // the last slice after OnDisable
    std::vector<float> buoy_;  // buoyancyData's copy of the held slice
    bool buoy_valid_ = false;
    long requested_ = 0, completed_ = 0;

    // bytes of one ring slot: a readback slice, or probe_cap_ query results
    size_t SliceBytes() const {
        if (readback == Readback::Probes) return probe_cap_ * 32;
        return (size_t)texturesSize * texturesSize * (readback == Readback::Height ? 4 : 16);
    }
    size_t HeldFloats() const { return readback == Readback::Probes ? held_count_ * 8 : SliceBytes() / 4; }

    void ApplyParams() {
        ocean_params p{windSpeed, windDirectionX, windDirectionY, gravity, fetch, depth};
        std::vector<ocean_cascade> cs;
        for (const auto& c : cascades) cs.push_back({c.wavelength, c.cutoffLow, c.cutoffHigh, c.swell, c.fade});
        check(ocean_set_params(ctx_, &p, cs.data()), "ocean_set_params");
    }

    // st: 1 done, < 0 request.hasError (data dropped, as the reference's callback does)
    void Complete(int st) {
        Pending p = readbacks_.front();
        readbacks_.pop_front();
        ocean_readback_release(p.req);
        if (st == 1) {
            // The reference copies every landed request out (request.GetData<Color>().ToArray(),
            // :295): Unity's NativeArray lives only inside the callback.  The pinned slot outlives
            // the request, so the slice stays in place and the slot leaves the ring until the next
            // landed readback replaces it (no 16 MiB host copy per frame at 1024^2).
            if (held_slot_) free_.push_back(held_slot_);
            held_slot_ = p.buf;
            held_ = static_cast<const float*>(p.buf);
            held_count_ = p.count;
            buoy_valid_ = false;
            ++completed_;
        } else {
            free_.push_back(p.buf);  // back to the ring
        }
    }
};

}  // namespace ocean_host
