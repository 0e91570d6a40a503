// abi_sequence: a compiled, non-Python host that plays a sequence of C-ABI calls in ONE process, the way a renderer
// calls the library once per frame for the life of the program.  abi_host makes one consumer call per process; this
// host makes the same blocking call again, other consumers between, requests in flight and a second context beside
// the first.  The sequences live in tests/test_gpu_host_sequences.py, which replays them through the Python binding
// and compares every result bit for bit; this program only interprets them.
//
//   abi_sequence <dir> <n> <cascades> <flags>
//
// Context 0 is the reference scene's first <cascades> cascades at N = <n>, seed 42, made through water_body.h's
// WaterBody (Awake .. OnDisable), so <flags> is OCEAN_F_MIPS, with OCEAN_F_VELOCITY or without.  <dir>/ops.txt has one
// op per line, blank-separated words; a name ending in .bin is a float32 file in <dir>; "-" stands for no file.
// Numbers are read by strtod and narrowed to float, as the Python binding narrows its doubles.
//
//   step <t>
//   grid <mode> <iterations> <lod> <x0> <z0> <dx> <dz> <nx> <ny>            ocean_surface_grid
//   camera <mode> <iterations> <steps> <refine> <width> <height> <camera.bin> <material.bin|->    ocean_camera
//   whitecaps <lod> <threshold> <x0> <z0> <dx> <dz> <nx> <ny> <capacity>    ocean_whitecaps
//   query_surface <mode> <iterations> <points.bin>
//   query_velocity <iterations> <points.bin>
//   raycast <iterations> <steps> <refine> <rays.bin>
//   body_buoyancy <mode> <iterations> <hull.bin> <bodies.bin>
//   body_dynamics <mode> <iterations> <law> <hull.bin> <bodies.bin> <motion.bin>
//   body_hydrostatics <iterations> <vertices.bin> <triangles.bin> <bodies.bin>    (triangles.bin holds int32)
//   sample_world <points.bin>
//   surface_bounds
//   read <texture> <cascade>                                                ocean_read of tile 0
//   read_height_async <cascade>     a request into pinned memory; its data is written when a later `wait` runs
//   grid_async <grid's arguments>   ocean_surface_grid_async, likewise
//   wait                            waits for every request in flight, oldest first, and releases it
//   ctx <k>                         the ops that follow go to context k (0 or 1)
//   ctx 1 <n> <cascades> <seed> <flags>    the same, making context 1 first: the scene's cascades, its own seed
//
// Op number k (from 0, every line counts) that produces data writes <dir>/out_<k>.bin, float32, exactly the bytes
// the library handed back; only a whitecap list's records past the W written, which ocean.h leaves unspecified, are
// cleared first.  Before every call the output buffer is filled with one NaN bit pattern (kSentinel), so the reader
// can tell a buffer the library never wrote from one it wrote zeros or wrong numbers to.  One JSON line on stdout:
//   {"hip_runtime": the path of the libamdhip64 mapped into this process, "hip_runtime_file": what it resolves to,
//    "ops": [{"k", "op", "ctx", "rc": the entry's return code, "words": float32 words of output, "sentinel": how
//    many of them still hold kSentinel after the call (a request: after its wait)}, ...]}
// A return code other than OCEAN_OK is recorded and the sequence goes on, except OCEAN_E_DEVICE, which ends it
// (exit 1).  A usage error (no arguments, an unknown op, a wrong number of words, unsupported flags) exits 2 before any
// device call.
#include <link.h>

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <sstream>
#include <string>

#include "water_body.h"

namespace {

constexpr uint32_t kSentinel = 0x7fc5ea5eu;  // a quiet NaN no kernel of the library produces

struct Op {
    std::string name;
    std::vector<std::string> args;
};

struct OpShape {
    const char* name;
    int argc;
};
const OpShape kOps[] = {{"step", 1},          {"grid", 9},          {"camera", 8},        {"whitecaps", 9},
                        {"query_surface", 3}, {"query_velocity", 2}, {"raycast", 4},       {"body_buoyancy", 4},
                        {"body_dynamics", 6}, {"body_hydrostatics", 4}, {"sample_world", 1},  {"surface_bounds", 0}, {"read", 2},
                        {"read_height_async", 1}, {"grid_async", 9}, {"wait", 0}};

int usage(const char* argv0, const std::string& why) {
    std::fprintf(stderr, "usage: %s <dir> <n> <cascades> <flags>   (plays <dir>/ops.txt; see the head of abi_sequence.cpp)\n%s\n",
                 argv0, why.c_str());
    return 2;
}

bool flags_supported(unsigned flags) { return (flags & ~(unsigned)OCEAN_F_VELOCITY) == OCEAN_F_MIPS; }

// "" when the line is a known op with the right number of words, else what is wrong with it
std::string check_op(const Op& op) {
    if (op.name == "ctx") {
        if (op.args.size() != 1 && op.args.size() != 5) return "ctx takes <k> or <k> <n> <cascades> <seed> <flags>";
        const int k = std::atoi(op.args[0].c_str());
        if (k != 0 && k != 1) return "ctx: context 0 or 1";
        if (op.args.size() == 5 && k != 1) return "ctx: only context 1 is made by an op";
        if (op.args.size() == 5 && !flags_supported((unsigned)std::strtoul(op.args[4].c_str(), nullptr, 0)))
            return "ctx: flags must be OCEAN_F_MIPS, with OCEAN_F_VELOCITY or without";
        return "";
    }
    for (const OpShape& s : kOps)
        if (op.name == s.name)
            return (int)op.args.size() == s.argc ? "" : op.name + " takes " + std::to_string(s.argc) + " words";
    return "unknown op " + op.name;
}

int find_runtime(struct dl_phdr_info* info, size_t, void* data) {
    if (info->dlpi_name && std::strstr(info->dlpi_name, "libamdhip64")) {
        *static_cast<std::string*>(data) = info->dlpi_name;
        return 1;
    }
    return 0;
}

std::string json_string(const std::string& s) {
    std::string o = "\"";
    for (char c : s) {
        if (c == '"' || c == '\\') o += '\\';
        o += c;
    }
    return o + "\"";
}

void fill_sentinel(float* p, size_t words) {
    for (size_t i = 0; i < words; ++i) std::memcpy(p + i, &kSentinel, 4);
}
size_t count_sentinel(const float* p, size_t words) {
    size_t c = 0;
    for (size_t i = 0; i < words; ++i) {
        uint32_t u;
        std::memcpy(&u, p + i, 4);
        c += u == kSentinel;
    }
    return c;
}

std::vector<float> read_bin(const std::string& path) {
    std::ifstream f(path, std::ios::binary | std::ios::ate);
    if (!f) throw std::runtime_error("cannot read " + path);
    const std::streamsize bytes = f.tellg();
    std::vector<float> v((size_t)bytes / 4);
    f.seekg(0);
    f.read(reinterpret_cast<char*>(v.data()), (std::streamsize)(v.size() * 4));
    return v;
}

void write_bin(const std::string& path, const float* data, size_t count) {
    FILE* f = std::fopen(path.c_str(), "wb");
    if (!f || std::fwrite(data, sizeof(float), count, f) != count) throw std::runtime_error("cannot write " + path);
    std::fclose(f);
}

float num(const std::string& s) { return (float)std::strtod(s.c_str(), nullptr); }
int integer(const std::string& s) { return (int)std::strtol(s.c_str(), nullptr, 0); }

struct Result {
    std::string op;
    int ctx = 0, rc = OCEAN_OK;
    size_t words = 0, sentinel = 0;
};

struct Pending {
    size_t k;
    ocean_readback* req;
    float* buf;  // pinned (ocean_host_alloc)
    size_t words;
};

// the six numbers of a grid and its mode, as `grid` and `grid_async` take them
struct Grid {
    int mode, iterations, nx, ny;
    float lod, x0, z0, dx, dz;
    size_t words;
    explicit Grid(const std::vector<std::string>& a)
        : mode(integer(a[0])), iterations(integer(a[1])), nx(integer(a[7])), ny(integer(a[8])), lod(num(a[2])),
          x0(num(a[3])), z0(num(a[4])), dx(num(a[5])), dz(num(a[6])) {
        const bool valid = nx >= 1 && ny >= 1 && (long long)nx * ny <= OCEAN_GRID_MAX_NODES;
        words = valid ? (size_t)nx * ny * (mode == OCEAN_GRID_HEIGHTFIELD ? 1 : 8) : 0;
    }
};

void awake_scene(ocean_host::WaterBody& wb, int n, int cascades, uint64_t seed, unsigned flags) {
    // the reference scene (Assets/Scenes/Waves.unity:1305-1322; cascades :1431-1435, :470-474, :1249-1253 and the
    // unreferenced 4th :1572-1576), as abi_host.cpp
    const ocean_host::WaterCascade scene[4] = {
        {1530.0f, 1e12f, 1e-10f, 0.4f, 0.1f}, {1000.0f, 1e7f, 1e-7f, 0.3f, 0.2f},
        {201.0f, 1e6f, 1e-5f, 0.1f, 0.1f}, {34.0f, 10.0f, 0.001f, 0.4f, 0.1f}};
    wb.windSpeed = 8.0f;
    wb.windDirectionX = 1.0f;
    wb.windDirectionY = -1.0f;
    wb.gravity = 9.81f;
    wb.fetch = 50000.0f;
    wb.depth = 2560.0f;
    wb.texturesSize = n;
    wb.cascades.assign(scene, scene + std::min(std::max(cascades, 1), 4));
    wb.seed = seed;
    wb.velocity = (flags & OCEAN_F_VELOCITY) != 0;
    wb.readback = ocean_host::Readback::Probes;  // with no probes set the facade requests nothing of its own
    wb.maxReadbacksInFlight = 1;
    wb.probeCapacity = 1;
    wb.Awake();
}

}  // namespace

int main(int argc, char** argv) {
    if (argc != 5) return usage(argv[0], "four arguments");
    const std::string dir = argv[1];
    const int n0 = std::atoi(argv[2]), C0 = std::atoi(argv[3]);
    const unsigned flags0 = (unsigned)std::strtoul(argv[4], nullptr, 0);
    if (!flags_supported(flags0)) return usage(argv[0], "flags must be OCEAN_F_MIPS, with OCEAN_F_VELOCITY or without");
    std::vector<Op> ops;
    {
        std::ifstream f(dir + "/ops.txt");
        if (!f) return usage(argv[0], "cannot read " + dir + "/ops.txt");
        std::string line;
        while (std::getline(f, line)) {
            std::istringstream words(line);
            Op op;
            if (!(words >> op.name)) continue;  // a blank line is no op
            for (std::string w; words >> w;) op.args.push_back(w);
            const std::string why = check_op(op);
            if (!why.empty()) return usage(argv[0], "ops.txt line \"" + line + "\": " + why);
            ops.push_back(op);
        }
    }
    std::string runtime;
    dl_iterate_phdr(find_runtime, &runtime);
    std::string runtime_file = runtime;
    if (!runtime.empty()) {
        char real[PATH_MAX];
        if (realpath(runtime.c_str(), real)) runtime_file = real;
    }

    std::vector<Result> results(ops.size());
    std::vector<Pending> pending;
    bool stopped = false;
    int exit_code = 0;
    try {
        ocean_host::WaterBody body[2];
        awake_scene(body[0], n0, C0, 42, flags0);
        int cur = 0;
        for (size_t k = 0; k < ops.size() && !stopped; ++k) {
            const Op& op = ops[k];
            const std::vector<std::string>& a = op.args;
            Result& res = results[k];
            res.op = op.name;
            if (op.name == "ctx") {
                cur = integer(a[0]);
                if (a.size() == 5) {
                    if (body[1].Context()) throw std::runtime_error("ctx: context 1 exists already");
                    awake_scene(body[1], integer(a[1]), integer(a[2]), std::strtoull(a[3].c_str(), nullptr, 0),
                                (unsigned)std::strtoul(a[4].c_str(), nullptr, 0));
                }
                if (!body[cur].Context()) throw std::runtime_error("ctx: context 1 was never made");
                res.ctx = cur;
                continue;
            }
            res.ctx = cur;
            ocean_host::WaterBody& wb = body[cur];
            ocean_ctx* ctx = wb.Context();
            const int N = wb.texturesSize, C = (int)wb.cascades.size();
            auto file = [&](const std::string& name) { return read_bin(dir + "/" + name); };
            std::vector<float> out;  // a blocking op's results
            auto prepare = [&](size_t words) {
                out.resize(words);
                fill_sentinel(out.data(), words);
            };
            if (op.name == "step") {
                res.rc = ocean_step(ctx, num(a[0]));
            } else if (op.name == "wait") {
                for (Pending& p : pending) {
                    const int rc = ocean_readback_wait(p.req);
                    ocean_readback_release(p.req);
                    Result& r = results[p.k];
                    if (r.rc == OCEAN_OK) r.rc = rc;
                    r.sentinel = count_sentinel(p.buf, p.words);
                    if (rc == OCEAN_OK) write_bin(dir + "/out_" + std::to_string(p.k) + ".bin", p.buf, p.words);
                    ocean_host_free(p.buf);
                    if (rc != OCEAN_OK) res.rc = rc;
                }
                pending.clear();
            } else if (op.name == "read_height_async" || op.name == "grid_async") {
                const bool height = op.name == "read_height_async";
                Pending p{k, nullptr, nullptr, height ? (size_t)N * N : Grid(a).words};
                void* mem = nullptr;
                ocean_host::check(ocean_host_alloc(std::max<size_t>(p.words, 1) * 4, &mem), "ocean_host_alloc");
                p.buf = static_cast<float*>(mem);
                fill_sentinel(p.buf, p.words);
                res.words = p.words;
                if (height) {
                    res.rc = ocean_read_height_async(ctx, 0, integer(a[0]), p.buf, p.words * 4, &p.req);
                } else {
                    const Grid g(a);
                    res.rc = ocean_surface_grid_async(ctx, 0, g.mode, g.iterations, g.lod, g.x0, g.z0, g.dx, g.dz, g.nx, g.ny,
                                                      p.buf, p.words * 4, &p.req);
                }
                if (res.rc == OCEAN_OK) {
                    pending.push_back(p);
                } else {
                    res.sentinel = count_sentinel(p.buf, p.words);
                    ocean_host_free(p.buf);
                }
            } else {
                if (op.name == "grid") {
                    const Grid g(a);
                    prepare(g.words);
                    res.rc = ocean_surface_grid(ctx, 0, g.mode, g.iterations, g.lod, g.x0, g.z0, g.dx, g.dz, g.nx, g.ny,
                                                out.data(), out.size() * 4);
                } else if (op.name == "camera") {
                    const int mode = integer(a[0]), width = integer(a[4]), height = integer(a[5]);
                    const std::vector<float> camera = file(a[6]);
                    const std::vector<float> material = a[7] == "-" ? std::vector<float>() : file(a[7]);
                    if (camera.size() != OCEAN_CAMERA_FLOATS || (!material.empty() && material.size() != OCEAN_CAMERA_MATERIAL_FLOATS))
                        throw std::runtime_error("camera: camera is 14 floats, material 32 or none");
                    const bool valid = width >= 1 && height >= 1 && (long long)width * height <= OCEAN_CAMERA_MAX_PIXELS;
                    prepare(valid ? (size_t)width * height * (mode == OCEAN_CAMERA_HITS ? 8 : mode == OCEAN_CAMERA_RANGE ? 1 : 4)
                                  : 0);
                    res.rc = ocean_camera(ctx, 0, mode, integer(a[1]), integer(a[2]), integer(a[3]), camera.data(),
                                          material.empty() ? nullptr : material.data(), width, height, out.data(),
                                          out.size() * 4);
                } else if (op.name == "whitecaps") {
                    const int capacity = integer(a[8]);
                    prepare(((size_t)std::min(std::max(capacity, 0), OCEAN_WHITECAP_MAX_RECORDS) + 1) * 8);
                    res.rc = ocean_whitecaps(ctx, 0, num(a[0]), num(a[1]), num(a[2]), num(a[3]), num(a[4]), num(a[5]),
                                             integer(a[6]), integer(a[7]), capacity, out.data(), out.size() * 4);
                } else if (op.name == "query_surface") {
                    const std::vector<float> points = file(a[2]);
                    prepare(points.size() / 2 * 8);
                    res.rc = ocean_query_surface(ctx, 0, integer(a[0]), integer(a[1]), points.data(), (int)(points.size() / 2),
                                                 out.data());
                } else if (op.name == "query_velocity") {
                    const std::vector<float> points = file(a[1]);
                    prepare(points.size() / 2 * 8);
                    res.rc = ocean_query_velocity(ctx, 0, integer(a[0]), points.data(), (int)(points.size() / 2), out.data());
                } else if (op.name == "raycast") {
                    const std::vector<float> rays = file(a[3]);
                    prepare(rays.size() / 8 * 8);
                    res.rc = ocean_raycast(ctx, 0, integer(a[0]), integer(a[1]), integer(a[2]), rays.data(),
                                           (int)(rays.size() / 8), out.data());
                } else if (op.name == "body_buoyancy") {
                    const std::vector<float> hull = file(a[2]), bodies = file(a[3]);
                    prepare(bodies.size() / 10 * 8);
                    res.rc = ocean_body_buoyancy(ctx, 0, integer(a[0]), integer(a[1]), hull.data(), (int)(hull.size() / 5),
                                                 bodies.data(), (int)(bodies.size() / 10), out.data());
                } else if (op.name == "body_dynamics") {
                    const std::vector<float> hull = file(a[3]), bodies = file(a[4]), motion = file(a[5]);
                    if (motion.size() / 6 != bodies.size() / 10) throw std::runtime_error("body_dynamics: one motion per body");
                    prepare(bodies.size() / 10 * 16);
                    res.rc = ocean_body_dynamics(ctx, 0, integer(a[0]), integer(a[1]), integer(a[2]), hull.data(),
                                                 (int)(hull.size() / 5), bodies.data(), motion.data(),
                                                 (int)(bodies.size() / 10), out.data());
                } else if (op.name == "body_hydrostatics") {
                    // the indices travel as the bytes the file holds: `file` reads 4-byte words and changes none
                    const std::vector<float> vertices = file(a[1]), triangles = file(a[2]), bodies = file(a[3]);
                    prepare(bodies.size() / 10 * OCEAN_HULL_RECORD_FLOATS);
                    res.rc = ocean_body_hydrostatics(ctx, 0, integer(a[0]), vertices.data(), (int)(vertices.size() / 3),
                                                     triangles.data(), (int)(triangles.size() / 3), bodies.data(),
                                                     (int)(bodies.size() / 10), out.data());
                } else if (op.name == "sample_world") {
                    const std::vector<float> points = file(a[0]);
                    prepare(points.size() / 3 * 12);
                    res.rc = ocean_sample_world(ctx, 0, points.data(), (int)(points.size() / 3), out.data());
                } else if (op.name == "surface_bounds") {
                    prepare((size_t)C * 8);
                    res.rc = ocean_surface_bounds(ctx, 0, out.data(), out.size() * 4);
                } else {  // read
                    const int texture = integer(a[0]);
                    const bool two = texture == OCEAN_TEX_NOISE || (texture >= OCEAN_TEX_PLANE0 && texture <= OCEAN_TEX_PLANE3);
                    prepare((size_t)N * N * (two ? 2 : 4));
                    res.rc = ocean_read(ctx, texture, 0, integer(a[1]), out.data(), out.size() * 4);
                }
                res.words = out.size();
                res.sentinel = count_sentinel(out.data(), out.size());
                if (res.rc == OCEAN_OK) {
                    if (op.name == "whitecaps" && res.sentinel == 0) {  // unspecified in the library's output
                        uint32_t head[8];
                        ocean_host::WaterBody::WhitecapHeader(out, head);
                        const size_t written = std::min<size_t>(head[1], out.size() / 8 - 1);
                        std::fill(out.begin() + 8 * (written + 1), out.end(), 0.0f);
                    }
                    write_bin(dir + "/out_" + std::to_string(k) + ".bin", out.data(), out.size());
                }
            }
            if (res.rc == OCEAN_E_DEVICE) {  // the device failed: nothing more is started on it
                std::fprintf(stderr, "abi_sequence: op %zu (%s): %s\n", k, op.name.c_str(), ocean_last_error());
                stopped = true;
                exit_code = 1;
            }
        }
        for (Pending& p : pending) {  // a sequence that ended without its `wait`
            ocean_readback_release(p.req);
            ocean_host_free(p.buf);
        }
        pending.clear();
        body[1].OnDisable();
        body[0].OnDisable();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "abi_sequence: %s\n", e.what());
        exit_code = 1;
    }
    std::printf("{\"hip_runtime\": %s, \"hip_runtime_file\": %s, \"sentinel\": %u, \"ops\": [", json_string(runtime).c_str(),
                json_string(runtime_file).c_str(), kSentinel);
    for (size_t k = 0; k < results.size(); ++k) {
        const Result& r = results[k];
        std::printf("%s{\"k\": %zu, \"op\": %s, \"ctx\": %d, \"rc\": %d, \"words\": %zu, \"sentinel\": %zu}", k ? ", " : "", k,
                    json_string(r.op).c_str(), r.ctx, r.rc, r.words, r.sentinel);
    }
    std::printf("]}\n");
    return exit_code;
}
