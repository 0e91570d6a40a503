// abi_host: a compiled, non-Python host walking the reference's WaterBody lifecycle
// through the C ABI (water_body.h): Awake -> Update x F (a readback request every
// frame) -> GetWaterHeight -> OnValidate (re-init, foam kept) -> Update -> SampleWorld
// -> OnDisable.  tests/test_gpu_host.py runs it and checks every number it writes
// against the same sequence through the Python binding and against the oracle.
//
//   abi_host <outdir> <n> <cascades> <frames> [height|rgba|probes|buoyancy|velocity|rays|dynamics|whitecaps|camera|camera_bodies|camera_scene|sky|step|spray|hydrostatics]
//
// With step the host plays F frames on a velocity context and, behind each, advances a fleet of six boxes of 4 x 3
// probes by 4 substeps of 1/240 s through one WaterBody::StepBodies in its async form (surface mode, 4 steps,
// quadratic drag), each call fed by the one before; it writes hull.bin, props.bin (float32 [6][4]), step.bin (float32
// [8]), state0.bin (float32 [6][32], the first call's input) and step_out.bin (float32 [6][32], the
// last call's output); the summary line carries those records too ("records", %.9g: exact for fp32);
// tests/test_gpu_step_host.py checks them.
// With camera the host reads nothing back per frame: it runs F steps, then one WaterBody::Camera for a fixed camera of
// 45 x 37 pixels (2 fixed-point steps, 32 march steps, 6 bisections): the shaded picture under a fixed material; it
// writes camera.bin (float32 [14]), material.bin (float32 [32]) and color.bin (float32 [37][45][4]); the summary line
// carries the number of pixels of each status; tests/test_gpu_camera_host.py checks them.
// With camera_bodies it runs F steps, then one WaterBody::CameraBodies in OCEAN_CAMERA_HITS mode for the camera mode's
// camera and five boxes in its view, records 16 floats apart: one in the air, three afloat, one sunk; it writes camera.bin,
// box.bin (float32 [6]), bodies.bin (float32 [5][16]) and body_hits.bin (float32 [37][45][8]); the summary line carries
// the number of pixels of each status; tests/test_gpu_camera_bodies_host.py checks them.
// With camera_scene it runs F steps, then two WaterBody::CameraScene calls for the same camera and boxes as camera_bodies
// (records 16 floats apart) under the camera mode's material, in OCEAN_CAMERA_LINKS and in OCEAN_CAMERA_COLOR mode; it
// writes camera.bin, material.bin, box.bin, paint.bin (float32 [4]), optics.bin (float32 [6]), bodies.bin, scene_links.bin
// and scene_color.bin (float32 [37][45][4] each); the summary line carries the number of water pixels that are shadowed,
// that show a body through the water and that reflect one; tests/test_gpu_camera_scene_host.py checks them.
// With sky it does the same behind the atmosphere: WaterBody::Atmosphere at the sizes 12 x 20, 3 x 5 and 20 x 12, one
// SkyUpdate, and the camera in OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT mode under the light colour SkyUpdate returned;
// it writes transmittance.bin, multiscatter.bin, skyview.bin (float32 [h][w][4] each), sun.bin (float32 [3]),
// sun_color.bin (float32 [3]), camera.bin, material.bin and sky_color.bin (float32 [24][32][4]);
// tests/test_gpu_atmosphere_host.py checks them.
// With spray the host runs F steps on a velocity context, takes the whitecaps mode's list, and makes two
// WaterBody::Spray calls of four substeps (K = 2): one that spawns from the list into an empty pool of 8192, one that
// advances that pool without spawning.  It writes spray_emitters.bin (float32 [4097][8]), spray0.bin and spray1.bin
// (float32 [8193][8]: the header, the W particles, zeros); tests/test_gpu_spray_host.py checks them.
// With whitecaps the host reads nothing back per frame: it runs F steps on a velocity context, then one
// WaterBody::Whitecaps over a 101 x 101 grid (threshold 0.1, capacity 4096, lod 0) and writes whitecaps.bin (float32
// [4097][8]: the header, the W records, zeros); the summary line carries the header's T and W and the W records
// ("records", %.9g: exact for fp32); tests/test_gpu_whitecaps_host.py checks them.
// With rays the host reads nothing back per frame: it runs F steps, then one WaterBody::Raycast for six rays (4
// fixed-point steps, 32 march steps, 8 bisections) and one WaterBody::SurfaceBounds, and writes rays.bin (float32
// [6][8]), raycast.bin (float32 [6][8]) and bounds.bin (float32 [cascades][8]); the summary line carries both
// results too ("records", "bounds", %.9g: exact for fp32); tests/test_gpu_ray_host.py checks them.
// With dynamics the host runs the buoyancy mode's five boxes on a velocity context (OCEAN_F_VELOCITY): F steps, then
// one WaterBody::Dynamics with five fixed motions (surface mode, 4 steps, linear drag), and writes hull.bin,
// bodies.bin, motion.bin (float32 [5][6]) and dynamics.bin (float32 [5][16]); the summary line carries the records
// too ("records", %.9g: exact for fp32); tests/test_gpu_dynamics_host.py checks them.
// With velocity the host reads nothing back per frame either: it creates the context with OCEAN_F_VELOCITY, runs F
// steps, then one WaterBody::Velocity for five points (4 steps) and writes velocity_points.bin (float32 [5][2]) and
// velocity.bin (float32 [5][8]); the summary line carries the records too ("records", %.9g: exact for fp32);
// tests/test_gpu_velocity_host.py checks them.
// With buoyancy the host reads nothing back per frame: it runs F steps, then one WaterBody::Buoyancy for five
// boxes of 4 x 3 probes (surface mode, 4 steps) and writes hull.bin (float32 [12][5]), bodies.bin (float32
// [5][10]) and buoyancy.bin (float32 [5][8]); the summary line carries the records too ("records", %.9g: exact
// for fp32); tests/test_gpu_body_host.py checks them.
// With hydrostatics the host reads nothing back per frame: it runs F steps, then one WaterBody::Hydrostatics for five
// boxes of the mesh of the box 2 x 1 x 3 (8 vertices, 12 triangles; 4 steps) and writes vertices.bin (float32 [8][3]),
// triangles.bin (int32 [12][3]), bodies.bin (float32 [5][10]) and hydrostatics.bin (float32 [5][16]); the summary line
// carries the records too ("records", %.9g: exact for fp32); tests/test_gpu_hull_host.py checks them.
// With probes the host reads no slice back: it sets five probes, runs F Updates (one surface query per
// frame, water_body.h Readback::Probes) and writes probe_heights.bin (float32 [F][5]: ProbeHeights after
// each Update, zeros before any query has landed), probe_results.bin (float32 [5][8]: the last query,
// after WaitForReadbacks) and the summary line; tests/test_gpu_query_host.py checks them.
// The readback mode (water_body.h Readback) defaults to height.  Writes <outdir>/buoyancy0.bin
// (buoyancyData after the first F frames, float32 [n][n] heights, or [n][n][4] with rgba),
// buoyancy1.bin (after OnValidate + one frame), heights.bin (float32
// [F][4]: GetWaterHeight at 4 world points after each Update), sample.bin (float32
// [8][12], SampleWorld of 8 points) and prints one JSON summary line.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <string>

#include "water_body.h"

namespace {

void write_bin(const std::string& path, const float* data, size_t count) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, sizeof(float), count, f) != count) {
        std::fprintf(stderr, "cannot write %s\n", path.c_str());
        std::exit(2);
    }
    std::fclose(f);
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5 && argc != 6) {
        std::fprintf(stderr, "usage: %s <outdir> <n> <cascades> <frames> [height|rgba|probes|buoyancy|velocity|rays|dynamics|whitecaps|camera|camera_bodies|camera_scene|sky|step|spray|hydrostatics]\n", argv[0]);
        return 2;
    }
    const std::string mode = argc == 6 ? argv[5] : "height";
    if (mode != "height" && mode != "rgba" && mode != "probes" && mode != "buoyancy" && mode != "velocity" &&
        mode != "rays" && mode != "dynamics" && mode != "whitecaps" && mode != "camera" && mode != "camera_bodies" &&
        mode != "camera_scene" && mode != "sky" && mode != "step" && mode != "spray" && mode != "hydrostatics") {
        std::fprintf(stderr, "usage: readback mode must be height, rgba, probes, buoyancy, velocity, rays, dynamics, whitecaps, camera, camera_bodies, camera_scene, sky, step, spray or hydrostatics\n");
        return 2;
    }
    const std::string out = argv[1];
    const int n = std::atoi(argv[2]), C = std::atoi(argv[3]), F = std::atoi(argv[4]);
    // the reference scene (Assets/Scenes/Waves.unity:1305-1322; cascades :1431-1435,
    // :470-474, :1249-1253 and the unreferenced 4th :1572-1576)
    const ocean_host::WaterCascade scene[4] = {
        {1530.0f, 1e12f, 1e-10f, 0.4f, 0.1f}, {1000.0f, 1e7f, 1e-7f, 0.3f, 0.2f},
        {201.0f, 1e6f, 1e-5f, 0.1f, 0.1f}, {34.0f, 10.0f, 0.001f, 0.4f, 0.1f}};
    try {
        ocean_host::WaterBody wb;
        wb.windSpeed = 8.0f;
        wb.windDirectionX = 1.0f;
        wb.windDirectionY = -1.0f;
        wb.gravity = 9.81f;
        wb.fetch = 50000.0f;
        wb.depth = 2560.0f;
        wb.texturesSize = n;
        wb.cascades.assign(scene, scene + (C < 4 ? C : 4));
        wb.seed = 42;
        if (mode == "buoyancy" || mode == "dynamics") {
            // a box of 4 x 3 cells (x fastest, then z), one layer: cell centres of [-1/2, 1/2]^3
            std::vector<float> hull;
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 4; ++i) {
                    const float cell[5] = {((float)i + 0.5f) / 4.0f - 0.5f, 0.0f, ((float)k + 0.5f) / 3.0f - 0.5f, 1.0f,
                                           1.0f / 12.0f};
                    hull.insert(hull.end(), cell, cell + 5);
                }
            // five boxes: origin, body -> world quaternion (x, y, z, w), scale
            const std::vector<float> bodies = {
                0.0f,    0.0f,   0.0f,     0.0f,  0.0f,  0.0f,  1.0f,  4.0f, 1.0f,  2.0f,
                37.5f,   0.25f,  -12.25f,  0.5f,  0.5f,  0.5f,  0.5f,  3.0f, 2.0f,  3.0f,
                -410.0f, -0.5f,  250.75f,  0.0f,  0.0f,  0.6f,  0.8f,  6.0f, 1.5f,  2.5f,
                1e4f,    0.125f, -3333.0f, 0.28f, 0.0f,  0.0f,  0.96f, 2.0f, 0.75f, 8.0f,
                -0.5f,   -0.25f, (float)n, 0.0f,  -0.6f, 0.0f,  0.8f,  5.0f, 3.0f,  1.0f};
            // five motions: world linear velocity of the origin, world angular velocity (dynamics mode)
            const std::vector<float> motion = {
                0.0f,  0.0f,   0.0f,  0.0f,  0.0f,   0.0f,
                1.0f,  2.0f,   -3.0f, 0.0f,  0.0f,   0.0f,
                0.0f,  0.0f,   0.0f,  0.0f,  1.0f,   0.0f,
                -2.5f, 0.125f, 4.0f,  0.25f, -0.5f,  0.75f,
                0.5f,  -1.0f,  0.25f, -1.5f, 0.125f, 0.0f};
            const bool dynamics = mode == "dynamics";
            wb.velocity = dynamics;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> rec = dynamics ? wb.Dynamics(hull, bodies, motion) : wb.Buoyancy(hull, bodies);
            write_bin(out + "/hull.bin", hull.data(), hull.size());
            write_bin(out + "/bodies.bin", bodies.data(), bodies.size());
            if (dynamics) write_bin(out + "/motion.bin", motion.data(), motion.size());
            write_bin(out + (dynamics ? "/dynamics.bin" : "/buoyancy.bin"), rec.data(), rec.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"probes\": %zu, \"bodies\": %zu, \"records\": [", F, n,
                        (int)wb.cascades.size(), hull.size() / 5, bodies.size() / 10);
            for (size_t i = 0; i < rec.size(); ++i) std::printf("%s%.9g", i ? ", " : "", rec[i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        if (mode == "hydrostatics") {
            // the box 2 x 1 x 3 as a closed mesh: corner ix + 2 iy + 4 iz, each face two triangles wound outward
            std::vector<float> vertices;
            for (int k = 0; k < 8; ++k) {
                const float corner[3] = {(k & 1) ? 1.0f : -1.0f, (k & 2) ? 0.5f : -0.5f, (k & 4) ? 1.5f : -1.5f};
                vertices.insert(vertices.end(), corner, corner + 3);
            }
            const int faces[6][4] = {{0, 4, 6, 2}, {1, 3, 7, 5}, {0, 1, 5, 4}, {2, 6, 7, 3}, {0, 2, 3, 1}, {4, 5, 7, 6}};
            std::vector<int> triangles;
            for (const auto& q : faces) {
                const int two[6] = {q[0], q[1], q[2], q[0], q[2], q[3]};
                triangles.insert(triangles.end(), two, two + 6);
            }
            // five boxes across the surface: origin, body -> world quaternion (x, y, z, w), scale
            const std::vector<float> bodies = {
                0.0f,    0.0f,   0.0f,     0.0f,  0.0f,  0.0f,  1.0f,  1.0f, 1.0f,  1.0f,
                37.5f,   0.25f,  -12.25f,  0.5f,  0.5f,  0.5f,  0.5f,  1.5f, 2.0f,  0.5f,
                -410.0f, -0.5f,  250.75f,  0.0f,  0.0f,  0.6f,  0.8f,  2.0f, 1.5f,  1.0f,
                1e4f,    0.125f, -3333.0f, 0.28f, 0.0f,  0.0f,  0.96f, 1.0f, 0.75f, 2.0f,
                -0.5f,   -0.25f, (float)n, 0.0f,  -0.6f, 0.0f,  0.8f,  0.5f, 3.0f,  1.0f};
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> rec = wb.Hydrostatics(vertices, triangles, bodies);
            write_bin(out + "/vertices.bin", vertices.data(), vertices.size());
            static_assert(sizeof(int) == sizeof(float), "triangles.bin is written as 4-byte words");
            write_bin(out + "/triangles.bin", reinterpret_cast<const float*>(triangles.data()), triangles.size());
            write_bin(out + "/bodies.bin", bodies.data(), bodies.size());
            write_bin(out + "/hydrostatics.bin", rec.data(), rec.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"vertices\": %zu, \"triangles\": %zu, \"bodies\": %zu, \"records\": [",
                        F, n, (int)wb.cascades.size(), vertices.size() / 3, triangles.size() / 3, bodies.size() / 10);
            for (size_t i = 0; i < rec.size(); ++i) std::printf("%s%.9g", i ? ", " : "", rec[i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        if (mode == "step") {
            const int substeps = 4;
            // a box of 4 x 3 cells (x fastest, then z), one layer, as the buoyancy mode's
            std::vector<float> hull;
            for (int k = 0; k < 3; ++k)
                for (int i = 0; i < 4; ++i) {
                    const float cell[5] = {((float)i + 0.5f) / 4.0f - 0.5f, 0.0f, ((float)k + 0.5f) / 3.0f - 0.5f, 1.0f,
                                           1.0f / 12.0f};
                    hull.insert(hull.end(), cell, cell + 5);
                }
            // six boxes: origin, quaternion (x, y, z, w), scale, linear and angular velocity; the record behind is zero
            const float fleet[6][16] = {
                {0.0f,    0.0f,   0.0f,     0.0f,  0.0f,  0.0f,  1.0f,  4.0f, 1.0f,  2.0f, 0.0f,  0.0f,   0.0f,  0.0f,  0.0f,   0.0f},
                {37.5f,   0.25f,  -12.25f,  0.5f,  0.5f,  0.5f,  0.5f,  3.0f, 2.0f,  3.0f, 1.0f,  2.0f,   -3.0f, 0.0f,  0.0f,   0.0f},
                {-410.0f, -0.5f,  250.75f,  0.0f,  0.0f,  0.6f,  0.8f,  6.0f, 1.5f,  2.5f, 0.0f,  0.0f,   0.0f,  0.0f,  1.0f,   0.0f},
                {1e4f,    0.125f, -3333.0f, 0.28f, 0.0f,  0.0f,  0.96f, 2.0f, 0.75f, 8.0f, -2.5f, 0.125f, 4.0f,  0.25f, -0.5f,  0.75f},
                {-0.5f,   -0.25f, (float)n, 0.0f,  -0.6f, 0.0f,  0.8f,  5.0f, 3.0f,  1.0f, 0.5f,  -1.0f,  0.25f, -1.5f, 0.125f, 0.0f},
                {12.0f,   30.0f,  7.0f,     0.0f,  0.0f,  0.0f,  1.0f,  1.0f, 1.0f,  1.0f, 0.0f,  0.0f,   0.0f,  0.0f,  0.0f,   0.5f}};
            std::vector<float> state(6 * 32, 0.0f);
            for (int b = 0; b < 6; ++b) std::copy(fleet[b], fleet[b] + 16, state.begin() + 32 * b);
            // inverse mass and inverse principal moments; the last body is deaf to torques
            const std::vector<float> props = {0.125f, 0.5f, 0.25f, 1.0f,  0.0625f, 0.125f, 0.125f, 0.125f, 0.05f, 0.1f, 0.02f, 0.2f,
                                              0.1f,   0.3f, 0.05f, 0.02f, 0.07f,   0.04f,  0.2f,   0.01f,  1.0f,  0.0f, 0.0f,  0.0f};
            // h, g, B, kd, kt, la, aa, 0
            const std::vector<float> step = {1.0f / 240.0f, 9.81f, 9.81f, 0.5f, 0.25f, 0.5f, 0.25f, 0.0f};
            wb.velocity = true;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            write_bin(out + "/state0.bin", state.data(), state.size());
            for (int f = 0; f < F; ++f) {
                wb.Update((float)f / 60.0f);
                state = wb.StepBodies(hull, state, props, step, substeps, 4, OCEAN_QUERY_SURFACE, OCEAN_DRAG_QUADRATIC, true);
            }
            write_bin(out + "/hull.bin", hull.data(), hull.size());
            write_bin(out + "/props.bin", props.data(), props.size());
            write_bin(out + "/step.bin", step.data(), step.size());
            write_bin(out + "/step_out.bin", state.data(), state.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"probes\": %zu, \"bodies\": %zu, \"substeps\": %d, "
                        "\"records\": [", F, n, (int)wb.cascades.size(), hull.size() / 5, state.size() / 32, substeps);
            for (size_t i = 0; i < state.size(); ++i) std::printf("%s%.9g", i ? ", " : "", state[i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        if (mode == "velocity") {
            // five positions (world x, world z): the probes mode's bodies
            const std::vector<float> points = {0.0f, 0.0f, 37.5f, -12.25f, -410.0f, 250.75f, 1e4f, -3333.0f, -0.5f, (float)n};
            wb.velocity = true;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> rec = wb.Velocity(points);
            write_bin(out + "/velocity_points.bin", points.data(), points.size());
            write_bin(out + "/velocity.bin", rec.data(), rec.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"points\": %zu, \"records\": [", F, n,
                        (int)wb.cascades.size(), points.size() / 2);
            for (size_t i = 0; i < rec.size(); ++i) std::printf("%s%.9g", i ? ", " : "", rec[i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        if (mode == "whitecaps") {
            // MeshGenerator's default plane as the region: 101 x 101 nodes 10 m apart around the origin
            const float threshold = 0.1f, x0 = -500.0f, z0 = -500.0f, dx = 10.0f, dz = 10.0f;
            const int nx = 101, ny = 101, capacity = 4096;
            wb.velocity = true;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> list = wb.Whitecaps(threshold, x0, z0, dx, dz, nx, ny, capacity);
            uint32_t head[8];
            ocean_host::WaterBody::WhitecapHeader(list, head);
            write_bin(out + "/whitecaps.bin", list.data(), list.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"nodes\": %u, \"capacity\": %u, \"selected\": %u, "
                        "\"written\": %u, \"records\": [", F, n, (int)wb.cascades.size(), head[2], head[3], head[0], head[1]);
            for (size_t i = 0; i < (size_t)head[1] * 8; ++i) std::printf("%s%.9g", i ? ", " : "", list[8 + i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        if (mode == "spray") {
            // the whitecaps mode's region and list, then two spray calls of four substeps of 1/240 s: the first spawns
            // from the list into an empty pool of 8192, the second advances that pool without spawning
            const float threshold = 0.1f, x0 = -500.0f, z0 = -500.0f, dx = 10.0f, dz = 10.0f;
            const int nx = 101, ny = 101, capacity = 4096, pool_capacity = 8192, substeps = 4, iterations = 2;
            // h, g, kd, wind, life, jet, lift, reserved
            const std::vector<float> spray = {1.0f / 240.0f, 9.81f, 0.5f, 3.0f, 0.0f, 1.0f, 2.0f, 1.0f,
                                              8.0f,          0.0f,  0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
            wb.velocity = true;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> list = wb.Whitecaps(threshold, x0, z0, dx, dz, nx, ny, capacity);
            const std::vector<float> first =
                wb.Spray(spray, ocean_host::WaterBody::EmptyPool(pool_capacity), list, substeps, iterations);
            const std::vector<float> second = wb.Spray(spray, first, {}, substeps, iterations);
            uint32_t h1[8], h2[8];
            ocean_host::WaterBody::WhitecapHeader(first, h1);
            ocean_host::WaterBody::WhitecapHeader(second, h2);
            write_bin(out + "/spray_emitters.bin", list.data(), list.size());
            write_bin(out + "/spray0.bin", first.data(), first.size());
            write_bin(out + "/spray1.bin", second.data(), second.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"capacity\": %u, \"candidates\": [%u, %u], "
                        "\"survivors\": [%u, %u], \"written\": [%u, %u]}\n", F, n, (int)wb.cascades.size(), h1[3], h1[2],
                        h2[2], h1[0], h2[0], h1[1], h2[1]);
            wb.OnDisable();
            return 0;
        }
        if (mode == "camera") {
            // an eye 30 m up that looks ahead and slightly down, so that the horizon crosses the image: the eye, the
            // direction through pixel (0, 0), its change per column and per row, t0, t1
            const int width = 45, height = 37;
            const std::vector<float> camera = {3.0f, 30.0f, -4.0f, -0.45f, 0.21f, 0.85f, 0.02f, 0.0f, 0.01f,
                                               0.0f,  -0.02f, 0.0f,  0.0f,   600.0f};
            // water colour, R0; Fresnel exponent and divisor of roughness 0.3, roughness, lod slope; EX, EY, environment
            // and sun strength; subsurface colour x intensity, foam threshold; foam colour, blending; light direction
            // (unit), light colour, horizon colour, zenith colour (ocean.h)
            const std::vector<float> material = {0.02f,  0.1f,  0.16f,  0.0203731f, 2.2308f, 4.72995f, 0.3f, 0.004f,
                                                 0.25f,  0.25f, 1.0f,   1.0f,       0.0f,    0.3f,     0.25f, 0.25f,
                                                 1.0f,   1.0f,  1.0f,   0.5f,       0.36f,   0.48f,    0.8f,  1.0f,
                                                 0.96f,  0.9f,  0.75f,  0.82f,      0.9f,    0.2f,     0.4f,  0.8f};
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> color = wb.Camera(camera, width, height, OCEAN_CAMERA_COLOR, material, 2, 32, 6);
            write_bin(out + "/camera.bin", camera.data(), camera.size());
            write_bin(out + "/material.bin", material.data(), material.size());
            write_bin(out + "/color.bin", color.data(), color.size());
            int status[3] = {0, 0, 0};
            for (int k = 0; k < width * height; ++k) ++status[(int)color[4 * k + 3]];
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"width\": %d, \"height\": %d, \"miss\": %d, "
                        "\"hit\": %d, \"submerged\": %d}\n", F, n, (int)wb.cascades.size(), width, height, status[0], status[1],
                        status[2]);
            wb.OnDisable();
            return 0;
        }
        if (mode == "camera_bodies") {
            const int width = 45, height = 37, stride = 16;
            const std::vector<float> camera = {3.0f, 30.0f, -4.0f, -0.45f, 0.21f, 0.85f, 0.02f, 0.0f, 0.01f,
                                               0.0f,  -0.02f, 0.0f,  0.0f,   600.0f};
            const std::vector<float> box = {-0.5f, -0.25f, -0.5f, 0.5f, 0.75f, 0.5f};
            // origin, quaternion (x, y, z, w), scale; the six floats behind them are not read
            const std::vector<float> bodies = {
                2.0f,   16.0f, 95.0f,  0.0f,  0.0f,  0.0f,  1.0f,  8.0f,  6.0f,  8.0f,  9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                -25.0f, 0.5f,  160.0f, 0.0f,  0.6f,  0.0f,  0.8f,  30.0f, 12.0f, 14.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                30.0f,  1.0f,  210.0f, 0.28f, 0.0f,  0.0f,  0.96f, 25.0f, 20.0f, 25.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                -5.0f,  -1.0f, 300.0f, 0.5f,  0.5f,  0.5f,  0.5f,  40.0f, 40.0f, 20.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                10.0f,  -30.0f, 120.0f, 0.0f, 0.0f,  0.0f,  1.0f,  30.0f, 10.0f, 30.0f};
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> hits = wb.CameraBodies(camera, width, height, box, {}, bodies, stride, OCEAN_CAMERA_HITS, {}, 2, 32, 6);
            write_bin(out + "/camera.bin", camera.data(), camera.size());
            write_bin(out + "/box.bin", box.data(), box.size());
            write_bin(out + "/bodies.bin", bodies.data(), bodies.size());
            write_bin(out + "/body_hits.bin", hits.data(), hits.size());
            int status[4] = {0, 0, 0, 0};
            for (int k = 0; k < width * height; ++k) ++status[(int)hits[8 * k + 3]];
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"width\": %d, \"height\": %d, \"miss\": %d, "
                        "\"hit\": %d, \"submerged\": %d, \"body\": %d}\n", F, n, (int)wb.cascades.size(), width, height,
                        status[0], status[1], status[2], status[3]);
            wb.OnDisable();
            return 0;
        }
        if (mode == "camera_scene") {
            const int width = 45, height = 37, stride = 16;
            const std::vector<float> camera = {3.0f, 30.0f, -4.0f, -0.45f, 0.21f, 0.85f, 0.02f, 0.0f, 0.01f,
                                               0.0f,  -0.02f, 0.0f,  0.0f,   600.0f};
            // the camera mode's material, but for a lower sun from the left: (-0.6, 0.35, 0.72) normalised
            const std::vector<float> material = {0.02f,  0.1f,  0.16f,  0.0203731f, 2.2308f, 4.72995f, 0.3f, 0.004f,
                                                 0.25f,  0.25f, 1.0f,   1.0f,       0.0f,    0.3f,     0.25f, 0.25f,
                                                 1.0f,   1.0f,  1.0f,   0.5f,       -0.599730f, 0.349843f, 0.719676f, 1.0f,
                                                 0.96f,  0.9f,  0.75f,  0.82f,      0.9f,    0.2f,     0.4f,  0.8f};
            const std::vector<float> box = {-0.5f, -0.25f, -0.5f, 0.5f, 0.75f, 0.5f};
            const std::vector<float> paint = {0.85f, 0.35f, 0.15f, 0.6f};
            // shadow colour and intensity, water fog density, reach of the secondary rays
            const std::vector<float> optics = {0.02f, 0.03f, 0.08f, 0.6f, 0.05f, 200.0f};
            const std::vector<float> bodies = {
                2.0f,   16.0f, 95.0f,  0.0f,  0.0f,  0.0f,  1.0f,  8.0f,  6.0f,  8.0f,  9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                -25.0f, 0.5f,  160.0f, 0.0f,  0.6f,  0.0f,  0.8f,  30.0f, 12.0f, 14.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                30.0f,  1.0f,  210.0f, 0.28f, 0.0f,  0.0f,  0.96f, 25.0f, 20.0f, 25.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                -5.0f,  -1.0f, 300.0f, 0.5f,  0.5f,  0.5f,  0.5f,  40.0f, 40.0f, 20.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f, 9.0f,
                10.0f,  -30.0f, 120.0f, 0.0f, 0.0f,  0.0f,  1.0f,  30.0f, 10.0f, 30.0f};
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> links = wb.CameraScene(camera, width, height, box, {}, optics, bodies, stride,
                                                            OCEAN_CAMERA_LINKS, material, 2, 32, 6);
            const std::vector<float> color = wb.CameraScene(camera, width, height, box, paint, optics, bodies, stride,
                                                            OCEAN_CAMERA_COLOR, material, 2, 32, 6);
            write_bin(out + "/camera.bin", camera.data(), camera.size());
            write_bin(out + "/material.bin", material.data(), material.size());
            write_bin(out + "/box.bin", box.data(), box.size());
            write_bin(out + "/paint.bin", paint.data(), paint.size());
            write_bin(out + "/optics.bin", optics.data(), optics.size());
            write_bin(out + "/bodies.bin", bodies.data(), bodies.size());
            write_bin(out + "/scene_links.bin", links.data(), links.size());
            write_bin(out + "/scene_color.bin", color.data(), color.size());
            int shadowed = 0, through = 0, mirrored = 0, water = 0;
            for (int k = 0; k < width * height; ++k) {
                if ((int)links[4 * k + 3] != OCEAN_RAY_HIT) continue;
                ++water;
                shadowed += links[4 * k] == 0.0f;
                through += links[4 * k + 1] >= 0.0f;
                mirrored += links[4 * k + 2] >= 0.0f;
            }
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"width\": %d, \"height\": %d, \"water\": %d, "
                        "\"shadowed\": %d, \"through\": %d, \"mirrored\": %d}\n", F, n, (int)wb.cascades.size(), width,
                        height, water, shadowed, through, mirrored);
            wb.OnDisable();
            return 0;
        }
        if (mode == "sky") {
            // the camera looks towards the sun, the horizon across the image and the sun's disc inside it
            const int width = 32, height = 24;
            const std::vector<float> sun = {0.3f, 0.25f, 0.9f};
            const std::vector<float> camera = {3.0f, 20.0f, -4.0f, -0.01f, 0.3f, 0.9f, 0.02f, 0.0f, 0.0f,
                                               0.0f, -0.03f, 0.0f, 0.0f, 600.0f};
            std::vector<float> material = {0.02f, 0.1f,  0.16f, 0.0203731f, 2.2308f, 4.72995f, 0.3f,  0.004f,
                                           0.25f, 0.25f, 1.0f,  1.0f,       0.0f,    0.3f,     0.25f, 0.25f,
                                           1.0f,  1.0f,  1.0f,  0.5f,       0.0f,    0.0f,     0.0f,  0.0f,
                                           0.0f,  0.0f,  0.0f,  0.0f,       0.0f,    0.0f,     0.0f,  0.0f};
            const float len = std::sqrt((sun[0] * sun[0] + sun[1] * sun[1]) + sun[2] * sun[2]);
            for (int k = 0; k < 3; ++k) material[20 + k] = sun[k] / len;
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            wb.Atmosphere(ocean_host::WaterBody::DefaultAtmosphere(), {12, 20, 3, 5, 20, 12});
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> rgb = wb.SkyUpdate(sun);
            for (int k = 0; k < 3; ++k) material[23 + k] = rgb[k];
            const std::vector<float> color =
                wb.Camera(camera, width, height, OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT, material, 2, 32, 6);
            const char* names[3] = {"/transmittance.bin", "/multiscatter.bin", "/skyview.bin"};
            int dims[6];
            for (int k = 0; k < 3; ++k) {
                const std::vector<float> lut = wb.AtmosphereLut(k, &dims[2 * k], &dims[2 * k + 1]);
                write_bin(out + names[k], lut.data(), lut.size());
            }
            write_bin(out + "/sun.bin", sun.data(), sun.size());
            write_bin(out + "/sun_color.bin", rgb.data(), rgb.size());
            write_bin(out + "/camera.bin", camera.data(), camera.size());
            write_bin(out + "/material.bin", material.data(), material.size());
            write_bin(out + "/sky_color.bin", color.data(), color.size());
            int status[3] = {0, 0, 0};
            for (int k = 0; k < width * height; ++k) ++status[(int)color[4 * k + 3]];
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"width\": %d, \"height\": %d, \"miss\": %d, "
                        "\"hit\": %d, \"submerged\": %d, \"dims\": [%d, %d, %d, %d, %d, %d]}\n", F, n, (int)wb.cascades.size(),
                        width, height, status[0], status[1], status[2], dims[0], dims[1], dims[2], dims[3], dims[4], dims[5]);
            wb.OnDisable();
            return 0;
        }
        if (mode == "rays") {
            // six rays (origin, direction, t0, t1): straight down, two slanted, one level, one upwards, one from below
            const std::vector<float> rays = {
                0.0f,    40.0f,  0.0f,     0.0f,  -1.0f,  0.0f,  0.0f, 80.0f,
                37.5f,   25.0f,  -12.25f,  0.6f,  -0.8f,  0.0f,  0.0f, 100.0f,
                -410.0f, 30.0f,  250.75f,  -2.0f, -1.0f,  3.0f,  0.0f, 60.0f,
                1e4f,    35.0f,  -3333.0f, 1.0f,  0.0f,   0.0f,  0.0f, 500.0f,
                -0.5f,   20.0f,  (float)n, 0.0f,  1.0f,   0.5f,  0.0f, 50.0f,
                12.0f,   -50.0f, 7.0f,     0.0f,  1.0f,   0.0f,  0.0f, 10.0f};
            wb.readback = ocean_host::Readback::Probes;  // with no probes set, Update requests nothing
            wb.Awake();
            for (int f = 0; f < F; ++f) wb.Update((float)f / 60.0f);
            const std::vector<float> rec = wb.Raycast(rays, 4, 32, 8);
            const std::vector<float> bounds = wb.SurfaceBounds();
            write_bin(out + "/rays.bin", rays.data(), rays.size());
            write_bin(out + "/raycast.bin", rec.data(), rec.size());
            write_bin(out + "/bounds.bin", bounds.data(), bounds.size());
            std::printf("{\"frames\": %d, \"n\": %d, \"cascades\": %d, \"rays\": %zu, \"records\": [", F, n,
                        (int)wb.cascades.size(), rays.size() / 8);
            for (size_t i = 0; i < rec.size(); ++i) std::printf("%s%.9g", i ? ", " : "", rec[i]);
            std::printf("], \"bounds\": [");
            for (size_t i = 0; i < bounds.size(); ++i) std::printf("%s%.9g", i ? ", " : "", bounds[i]);
            std::printf("]}\n");
            wb.OnDisable();
            return 0;
        }
        wb.readback = mode == "height"  ? ocean_host::Readback::Height
                      : mode == "rgba" ? ocean_host::Readback::Rgba
                                       : ocean_host::Readback::Probes;
        if (mode == "probes") {
            // five bodies; Update asks for the surface above each (surface mode, 4 steps: the facade's defaults)
            const std::vector<float> bodies = {0.0f,   0.0f, 0.0f,    37.5f,    1.0f, -12.25f, -410.0f, 0.0f,
                                               250.75f, 1e4f, -2.0f, -3333.0f, -0.5f, 0.0f,    (float)n};
            const size_t M = bodies.size() / 3;
            wb.probeCapacity = M;
            wb.SetProbes(bodies);
            wb.Awake();
            std::vector<float> heights;
            for (int f = 0; f < F; ++f) {
                wb.Update((float)f / 60.0f);
                std::vector<float> h = wb.ProbeHeights();
                h.resize(M, 0.0f);  // zeros before any query has landed
                heights.insert(heights.end(), h.begin(), h.end());
            }
            wb.WaitForReadbacks();
            write_bin(out + "/probe_heights.bin", heights.data(), heights.size());
            const std::vector<float> last = wb.ProbeResults();
            write_bin(out + "/probe_results.bin", last.data(), last.size());
            std::printf("{\"frames\": %d, \"requested\": %ld, \"completed\": %ld, \"n\": %d, \"cascades\": %d, "
                        "\"probes\": %zu}\n", F, wb.requested(), wb.completed(), n, (int)wb.cascades.size(), M);
            wb.OnDisable();
            return 0;
        }
        wb.Awake();
        const float probe[4][2] = {{0.0f, 0.0f}, {-(float)n / 2, -(float)n / 2}, {(float)n / 2 - 1, 50.0f}, {500.0f, -500.0f}};
        std::vector<float> heights;
        for (int f = 0; f < F; ++f) {
            wb.Update((float)f / 60.0f);
            for (auto& p : probe) heights.push_back(wb.GetWaterHeight(p[0], p[1]));
        }
        wb.WaitForReadbacks();
        {
            const std::vector<float>& buoy = wb.buoyancyData();
            write_bin(out + "/buoyancy0.bin", buoy.data(), buoy.size());
        }
        write_bin(out + "/heights.bin", heights.data(), heights.size());
        wb.windSpeed = 12.0f;
        wb.OnValidate();
        wb.Update(0.5f);
        wb.WaitForReadbacks();
        {
            const std::vector<float>& buoy = wb.buoyancyData();
            write_bin(out + "/buoyancy1.bin", buoy.data(), buoy.size());
        }
        std::vector<float> pts;
        for (int i = 0; i < 8; ++i) {
            pts.push_back(-300.0f + 97.5f * i);
            pts.push_back(40.0f - 13.25f * i);
            pts.push_back(0.5f * i);
        }
        const std::vector<float> s = wb.SampleWorld(pts);
        write_bin(out + "/sample.bin", s.data(), s.size());
        std::printf("{\"frames\": %d, \"requested\": %ld, \"completed\": %ld, \"n\": %d, \"cascades\": %d}\n", F + 1,
                    wb.requested(), wb.completed(), n, (int)wb.cascades.size());
        wb.OnDisable();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "abi_host: %s\n", e.what());
        return 1;
    }
    return 0;
}
