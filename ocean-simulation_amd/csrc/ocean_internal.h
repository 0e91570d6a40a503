// Internal declarations shared by the C-ABI layer (abi_*.cpp) and the HIP kernel translation
// units (every csrc/*.hip): the launch wrapper, the device view of a context and one launch_*
// function per kernel family.  Not part of the ABI.
#pragma once

#include <hip/hip_ext.h>
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <type_traits>

#include "frame_plan.h"  // pass_*_supported: which sizes each pass family is built for
#include "ocean/ocean.h"

namespace ocean {

// Kernel timing (ocean_set_kernel_timing): the C-ABI layer points this thread's slot at an
// event pair around one entry point's launches; every kernel launch goes through launch(),
// which attaches the pair to the dispatch itself (hipExtLaunchKernel: start of the first
// kernel, end of the last), so the measured time is the kernels' own, as rocprofv3 reports it,
// with no marker packets between them.
struct LaunchEvents {
    hipEvent_t start, stop;
    bool launched;
};
LaunchEvents*& launch_events();  // thread-local slot, launch.cpp
// Host pointer of the kernel this thread launched last (ocean_kernel_name reports its symbol).
const void*& last_kernel();  // thread-local slot, launch.cpp

template <class F, class... Args>
inline void launch(F kernel, dim3 grid, dim3 block, uint32_t shmem, hipStream_t s, Args... args) {
    last_kernel() = (const void*)kernel;
    LaunchEvents* e = launch_events();
    hipExtLaunchKernelGGL(kernel, grid, block, shmem, s, e && !e->launched ? e->start : nullptr,
                          e ? e->stop : nullptr, 0, args...);
    if (e) e->launched = true;
}

// From a runtime value to a template argument: f(std::integral_constant<int, V>{}) for the V among Vs that equals
// `value`; false, and no call, when none does.  A launcher states its kernel's argument list once, in a generic
// lambda, and the kernels instantiated are those of Vs (grid.hip, view.hip, body.hip).
template <int... Vs, class F>
inline bool with_constant(int value, F&& f) {
    return ((value == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

constexpr int kMaxCascades = 5;  // the consumer shader caps cascades at 5 (Water.shader:139)

// Device-side view of one context: every texture of every (tile, cascade) unit.
// unit u = tile * C + cascade; each texture is [u][y][x] (see include/ocean/ocean.h).
struct DevView {
    int n;       // grid side N
    int logn;    // log2 N
    int C;       // cascades
    int T;       // tiles
    int units;   // T * C
    int planes;  // 4 (full) or 2 (displacement only)
    bool normals;
    int max_groups;  // OCEAN_MAX_GROUPS: cap of every persistent launch grid (capped_grid), 0 = none.  Host only;
                     // it lies in the padding after `normals`, so the kernels' argument layout is unchanged
    const float2* noise;  // [T][N][N]
    float4* h0;           // [U][N][N]
    float2* h0k;          // [U][N][N] h0(k) alone (= h0.xy); the mirror-pair row pass reads h0(k) and h0(-k) here
    float4* waves;        // [U][N][N]
    float2* plane[4];     // [U][N][N] each; one allocation, plane[p] = plane[0] + p * plane_stride
    size_t plane_stride;  // elements between consecutive planes (U * N * N)
    float4* disp;         // [U][N][N]
    float4* deriv;        // [U][N][N] (full only)
    float4* turb;         // [U][N][N] (full only)
    float4* normal;       // [U][N][N] (normals only)
    const float2* tw;     // [N + 128]: exp(+2 pi i m / N), m < N; then T1[64] = exp(2 pi i lo / N),
                          // T2[64] = exp(2 pi i 64 hi / N) (two-level table for N > 1024)
    const float* casc;    // [C][5] wavelength, cutoff_low, cutoff_high, swell, fade (device)
    float gravity;        // for the per-frame wave-data recompute (fused row pass)
    int tile_w;           // width W of the tile-major layouts below: inter_w(N), or 4 for small jobs
    float2* tplane;       // fused intermediate, P planes x [K][N/W][N][W] (tile-major), stride inter_stride;
                          // K = the units of one chunk of a frame (frame_plan.h chunk_units): every chunk
                          // reuses the same region, so its lines are rewritten in the Infinity Cache
                          // instead of being written back to HBM once per unit
    size_t inter_stride;  // elements between consecutive planes of tplane (K * N * N)
    float* foam;          // foam state, [U][N/W][N][W] (tile-major); TURB is its broadcast RGBA image
    float2* qside;        // three-plane frame (fftq.hip): per unit of a chunk, d0 [N] then srow [N]
    float4* deriv_mips;   // OCEAN_F_MIPS: per slice, levels 1..log2 N concatenated (mip_chain texels)
    float4* turb_mips;
    size_t mip_chain;     // texels per slice chain: sum over L >= 1 of (N >> L)^2
    // column band (ocean_set_column_band): the fused passes store / transform / fill
    // columns x0 <= x < x0 + nx only (rows are still transformed whole); x0 and nx are
    // multiples of the tile widths, full band = (0, N)
    int x0, nx;
    int c0;  // cascade of unit 0 of this view (a sub-view of a unit chunk may start mid-tile)
    // column parity (ocean_set_column_parity): the context computes the columns x = xstr * m + xpar and
    // stores column x at texture / intermediate column m < N / xstr; xstr = 1, xpar = 0 when off
    int xstr, xpar;
    // pass BQ writes DISP with default-policy stores instead of nontemporal ones: the slice stays in the
    // Infinity Cache and is written back while the next pass A runs, when HBM has headroom.  Set by the host
    // where the frame's re-read set plus DISP fits the cache (frame_plan.h disp_fits_cache).
    bool disp_cached;
    // Deferred TURB (frame_plan.h defer_turb).  turb_defer: pass BQ does not store TURB; the foam state alone
    // carries the frame's foam (host only: it selects the kernel).  turb_foam: the float4 array is stale, so the
    // level-0 TURB taps of the point consumers read the foam state (sample_filter.h).  Both lie in the padding
    // after disp_cached.
    bool turb_defer;
    bool turb_foam;
};

static_assert(sizeof(DevView) == 240, "DevView is a kernel argument: a new field changes every kernel's argument layout");

struct SpectrumParams {
    float wind_speed, wind_dir_x, wind_dir_y, gravity, fetch, depth;
};

// launch.cpp
// Resident workgroups per CU of `kernel` at `threads` lanes (hipOccupancyMaxActiveBlocksPerMultiprocessor,
// at least 1) and the device's CU count, cached per device (and kernel): the queries cost microseconds
// of host time, paid once instead of per launch (small jobs issue a launch every few microseconds).
int resident_per_cu(const void* kernel, int threads);
int device_cus();
// The grid of a persistent launch under OCEAN_MAX_GROUPS: at most max_groups workgroups when the cap is
// positive.  Every persistent kernel walks item = blockIdx.x, += gridDim.x and no kernel synchronises across
// workgroups, so any grid >= 1 computes the same texels; a small one makes every workgroup's loop iterate.
inline int capped_grid(int g, int max_groups) { return max_groups > 0 && g > max_groups ? max_groups : g; }
// The item loop of a persistent kernel and the grid that runs it: min(items, resident slots of the device),
// where a CU holds what the kernel's occupancy allows or at most max_per_cu (> 0) workgroups.
// group > 1 (XCD-grouped column launches, fft2.hip): a multiple of `group` workgroups, so that the pieces of a
// tile sit on blocks b, b + 8, ... at every step of the item loop (their items are a multiple of it too).  That
// placement is speed only (k_cols2), so the OCEAN_MAX_GROUPS cap applies after it and need not keep it.
struct Items {
    int count, max_groups, group = 1, max_per_cu = 0;
};
template <class F, class... Args>
inline hipError_t launch_items(F kernel, int threads, Items it, hipStream_t s, const Args&... args) {
    int per_cu = resident_per_cu((const void*)kernel, threads);
    if (it.max_per_cu > 0 && per_cu > it.max_per_cu) per_cu = it.max_per_cu;
    int g = device_cus() * per_cu;
    if (it.count < g) g = it.count;
    g -= g % it.group;
    launch(kernel, dim3(capped_grid(g, it.max_groups)), dim3(threads), 0, s, args...);
    return hipGetLastError();
}

hipError_t launch_init_spectrum(const DevView& v, const SpectrumParams& p, hipStream_t s);
hipError_t launch_conjugate(const DevView& v, hipStream_t s);
hipError_t launch_evolve(const DevView& v, float t, hipStream_t s);
hipError_t launch_fill(const DevView& v, hipStream_t s);
hipError_t launch_foam_import(const DevView& v, hipStream_t s);
// TURB <- (f, f, f, f) of the foam state, every unit (deferred TURB: the float4 array when an entry needs it)
hipError_t launch_turb_materialise(const DevView& v, hipStream_t s);
hipError_t launch_noise(const DevView& v, uint64_t seed, hipStream_t s);
// h0k = h0.xy (a context whose h0k is allocated after its spectrum: ocean_set_column_parity)
hipError_t launch_h0k_extract(const DevView& v, hipStream_t s);
// ext[u] (device, [units]) = the largest |y - N/2| over the rows y of unit u's h0k that hold a texel != 0
// (a NaN counts), -1 when the unit holds none
hipError_t launch_live_extent(const DevView& v, int* ext, hipStream_t s);

// fft2.hip: the operator IFFT (IFFT.InverseFastFourierTransform): persistent,
// software-pipelined row and column(+permute) launches, in place.
// Entries of the per-stage twiddle tables stored at tw + N + 128 (see fft_engine.h StageTw).
size_t stage_twiddle_entries(int n);
// Each launch covers `ups` consecutive unit-planes from `base` (plane p of unit u is unit-plane
// p * U + u of the one plane allocation), in place.
hipError_t launch_ifft_rows_v2(const DevView& v, float2* base, int ups, hipStream_t s);
hipError_t launch_ifft_cols_v2(const DevView& v, float2* base, int ups, hipStream_t s);
// N = 4096: the operator over `ups` consecutive unit-planes at `planes` (plane p of unit u is
// unit-plane p * U + u) with its column transform split by decimation in frequency into two 2048-point
// column transforms, in place (fft2.hip): part 0 = rows + fold onto the planes' own rows (k_rowsf),
// 1 = the column transforms + permute, both sub-planes of an XCD-paired 8-column tile per item (k_colsf_ip).
hipError_t launch_ifft_fold(const DevView& v, float2* planes, int ups, int part, hipStream_t s);

// fft3.hip: fused frame through the tile-major intermediate; the row pass
// recomputes wave data and feeds evolve straight into a radix-4/8 first stage;
// the column pass (N <= 1024) reads contiguous tiles and the compact foam state.
hipError_t launch_pass_a_v3(const DevView& v, float t, hipStream_t s);
hipError_t launch_pass_b_v3(const DevView& v, hipStream_t s);
// mips.hip: box-filter mip chains of DERIV and TURB (OCEAN_F_MIPS)
hipError_t launch_mips(const DevView& v, hipStream_t s);
// mips.hip: DISP.y of one slice compacted to float[N][N] (ocean_read_height_async); texels % 4 == 0
hipError_t launch_extract_height(const float4* disp_slice, float* dst, size_t texels, hipStream_t s);
// sample.hip: cascade-summed world sampling (Water.shader:314-348), device pointers
hipError_t launch_sample_world(const DevView& v, int tile, const float* pts, int count, float* out, hipStream_t s);
// query.hip: surface queries (ocean_query_surface*), device pointers: pts float[count][2], out float[count][8]
hipError_t launch_query_surface(const DevView& v, int tile, int mode, int iterations, const float* pts, int count,
                                float* out, hipStream_t s);
// grid.hip: surface grids (ocean_surface_grid*), device pointer: out float[ny][nx][8], or float[ny][nx] in
// OCEAN_GRID_HEIGHTFIELD mode; tile_w = the workgroup's tile width in nodes (grid_tile_supported)
bool grid_tile_supported(int tile_w);
hipError_t launch_surface_grid(const DevView& v, int tile, int mode, int iterations, float lod, float x0, float z0,
                               float dx, float dz, int nx, int ny, int tile_w, float* out, hipStream_t s);
// body.hip: buoyant bodies (ocean_body_buoyancy*), device pointers: hull float[probes][5], bodies float[count][10],
// out float[count][8]; body_segment_width = lanes per body (the smallest power of two >= probes, at most 64)
int body_segment_width(int probes);
hipError_t launch_body_buoyancy(const DevView& v, int tile, int mode, int iterations, const float* hull, int probes,
                                const float* bodies, int count, float* out, hipStream_t s);
// body.hip: the buoyancy record and the drag against the water's velocity (ocean_body_dynamics*), device pointers:
// vel = the context's VEL float4 [U][N][N], motion float[count][6], law OCEAN_DRAG_*, out float[count][16]
hipError_t launch_body_dynamics(const DevView& v, const float4* vel, int tile, int mode, int iterations, int law,
                                const float* hull, int probes, const float* bodies, const float* motion, int count,
                                float* out, hipStream_t s);
// body.hip: substeps of the rigid bodies behind that record (ocean_body_step*), device pointers: props float[count][4],
// state float[count][32], out float[count][32], which may be `state` itself; sp = the entry's eight `step` floats,
// which travel as a kernel argument
struct BodyStepParams {
    float p[OCEAN_BODY_STEP_FLOATS];
};
hipError_t launch_body_step(const DevView& v, const float4* vel, int tile, int mode, int iterations, int law, int substeps,
                            const BodyStepParams& sp, const float* hull, int probes, const float* props,
                            const float* state, int count, float* out, hipStream_t s);
// hull.hip: hydrostatic pressure over the wetted triangles of a mesh hull (ocean_body_hydrostatics*), device pointers:
// vertices float[nverts][3], triangles int[ntris][3] (an index outside [0, nverts) is clamped into it), bodies
// float[count][10], out float[count][16]
hipError_t launch_body_hydrostatics(const DevView& v, int tile, int iterations, const float* vertices, int nverts,
                                    const int* triangles, int ntris, const float* bodies, int count, float* out,
                                    hipStream_t s);
// velocity.hip: surface velocity (OCEAN_F_VELOCITY).  `scratch` is the context's two velocity planes, float2
// [2][U][N][N] plane-major: launch_evolve_velocity writes the packed planes of dh/dt at t there (from v.h0 and
// v.waves), the operator IFFT transforms them in place as 2 U unit-planes, launch_pack_velocity interleaves them
// into vel float4 [U][N][N] (streamed: nontemporal stores).  launch_query_velocity: ocean_query_velocity*,
// device pointers: pts float[count][2], out float[count][8].
hipError_t launch_evolve_velocity(const DevView& v, float2* scratch, float t, hipStream_t s);
hipError_t launch_pack_velocity(const DevView& v, const float2* scratch, float4* vel, bool streamed, hipStream_t s);
hipError_t launch_query_velocity(const DevView& v, const float4* vel, int tile, int iterations, const float* pts,
                                 int count, float* out, hipStream_t s);

// bounds.hip: surface bounds (ocean_surface_bounds*), device pointers: out float[C][8], the channel-wise
// (min xyzw, max xyzw) of the DISP slices of tile `tile`; partial: scratch of bounds_partial_floats(C) floats
// (pass 1 writes at most kBoundsMaxGroups records per slice there, pass 2 folds them).  Both 16-B aligned.
constexpr int kBoundsMaxGroups = 256;
size_t bounds_partial_floats(int C);
hipError_t launch_surface_bounds(const DevView& v, int tile, float* partial, float* out, hipStream_t s);
// ray.hip: ray casts (ocean_raycast*), device pointers: rays float[count][8], out float[count][8]; bounds:
// the tile's float[C][8] of launch_surface_bounds for the air skip, or null to sample every node
hipError_t launch_raycast(const DevView& v, int tile, int iterations, int steps, int refine, const float* bounds,
                          const float* rays, int count, float* out, hipStream_t s);

// view.hip: camera views (ocean_camera*), device pointer: out float[height][width][8] (OCEAN_CAMERA_HITS), float
// [height][width] (_RANGE) or float[height][width][4] (_COLOR), 16-B aligned.  The camera's 14 and the material's 32
// floats of ocean.h travel as kernel arguments (the material is not read in the first two modes); bounds as
// launch_raycast takes them; tiled: a wave covers 8 x 8 pixels, else 64 consecutive pixels of the row-major image.
struct CameraRays {
    float c[OCEAN_CAMERA_FLOATS];
};
struct CameraMaterial {
    float m[OCEAN_CAMERA_MATERIAL_FLOATS];
};
hipError_t launch_camera(const DevView& v, int tile, int mode, int iterations, int steps, int refine, const float* bounds,
                         const CameraRays& cam, const CameraMaterial& mt, int width, int height, bool tiled, float* out,
                         hipStream_t s);

// atmosphere.hip: the atmosphere's look-up tables (ocean_atmosphere, ocean_sky_update), device pointers, float4 per
// texel, row-major [h][w].  The entry's 32 `params` floats travel as a kernel argument; `sun` is the unit direction
// towards the sun (host array of three).  Every width and height lies in [2, OCEAN_ATMOSPHERE_MAX_DIM].
struct AtmosphereParams {
    float p[OCEAN_ATMOSPHERE_FLOATS];
};
struct LutView {
    const float4* texels;
    int w, h;
};
hipError_t launch_transmittance(const AtmosphereParams& a, int w, int h, float4* lut, hipStream_t s);
hipError_t launch_multiscatter(const AtmosphereParams& a, const LutView& tr, int w, int h, float4* lut, hipStream_t s);
hipError_t launch_skyview(const AtmosphereParams& a, const LutView& tr, const LutView& ms, const float* sun, int w, int h,
                          float4* lut, hipStream_t s);
// view.hip: launch_camera's colour image with the sky of OCEAN_CAMERA_SKY_LUT: `sky` is the sky-view table and
// sun_size the atmosphere's params[26].  Its own kernel: the three kernels of launch_camera keep their arguments.
hipError_t launch_camera_sky(const DevView& v, int tile, int iterations, int steps, int refine, const float* bounds,
                             const CameraRays& cam, const CameraMaterial& mt, const LutView& sky, float sun_size, int width,
                             int height, bool tiled, float* out, hipStream_t s);
// view.hip: camera views with bodies (ocean_camera_bodies*): launch_camera's image, or launch_camera_sky's in the mode
// OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT (`sky` and sun_size are read in that mode only), with the boxes of `bodies`
// in front of the water: record b at bodies + b * stride floats, device pointer, may be null when count is 0.  The box's
// 6 and the paint's 4 floats of ocean.h travel as kernel arguments.  Always the tiled mapping.  cull: the per-tile
// bounding-sphere cull (false: every body reaches every pixel's slab test; the same image).
struct BodyBox {
    float b[6];
};
struct BodyPaint {
    float p[OCEAN_BODY_PAINT_FLOATS];
};
hipError_t launch_camera_bodies(const DevView& v, int tile, int mode, int iterations, int steps, int refine,
                                const float* bounds, const CameraRays& cam, const CameraMaterial& mt, const LutView& sky,
                                float sun_size, const BodyBox& box, const BodyPaint& paint, const float* bodies, int stride,
                                int count, bool cull, int width, int height, float* out, hipStream_t s);
// view.hip: camera views in which the water sees the bodies (ocean_camera_scene*): launch_camera_bodies' colour image
// with the bodies' shadows, reflections and fogged submerged parts at the water pixels, or the OCEAN_CAMERA_LINKS
// record of those decisions; mode is OCEAN_CAMERA_COLOR, OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT or
// OCEAN_CAMERA_LINKS, 16 B per pixel in each.  The six `optics` floats of ocean.h travel as a kernel argument.
// cull: both culls (false: every body reaches every ray's slab test; the same image).
struct SceneOptics {
    float o[OCEAN_SCENE_OPTICS_FLOATS];
};
hipError_t launch_camera_scene(const DevView& v, int tile, int mode, int iterations, int steps, int refine,
                               const float* bounds, const CameraRays& cam, const CameraMaterial& mt, const LutView& sky,
                               float sun_size, const BodyBox& box, const BodyPaint& paint, const SceneOptics& optics,
                               const float* bodies, int stride, int count, bool cull, int width, int height, float* out,
                               hipStream_t s);

// whitecaps.hip: whitecap emitters (ocean_whitecaps*), device pointers: out = (capacity + 1) records of 32 B, the
// header then the selected nodes of the grid in ascending node order, 16-B aligned; vel = the context's VEL or null
// (records carry a zero velocity); scratch: whitecap_scratch_bytes() bytes, 8-B aligned, the ballot masks of the
// largest grid then its per-chunk counts.  Three launches: count, scan, emit.
size_t whitecap_scratch_bytes();
hipError_t launch_whitecaps(const DevView& v, const float4* vel, int tile, float lod, float threshold, float x0, float z0,
                            float dx, float dz, int nx, int ny, int capacity, void* scratch, float* out, hipStream_t s);

// compact.hip: the scan between a compaction's count and emit launches (compact.h), one workgroup: counts[0 .. items)
// become exclusive offsets in place and `out` gets the header record (T, min(T, capacity), third, capacity, 0, 0, 0, 0),
// third = *nodes_dev when that is not null, else nodes.
hipError_t launch_compact_scan(unsigned* counts, unsigned items, unsigned nodes, const unsigned* nodes_dev,
                               unsigned capacity, float* out, hipStream_t s);

// spray.hip: spray particles (ocean_spray_step*), device pointers: pool and out = (capacity + 1) records of 32 B, the
// header then the particles, emitters = a whitecap list of (emit_capacity + 1) records or null with emit_capacity 0,
// all 16-B aligned; sp = the entry's sixteen `spray` floats, which travel as a kernel argument; bounds as
// launch_raycast takes them; scratch: spray_scratch_bytes(capacity, emit_capacity) bytes, 16-B aligned.  Three
// launches: step, scan, emit.
struct SprayParams {
    float p[OCEAN_SPRAY_FLOATS];
};
size_t spray_scratch_bytes(int capacity, int emit_capacity);
hipError_t launch_spray_step(const DevView& v, int tile, int iterations, int substeps, const SprayParams& sp,
                             const float* bounds, const float* pool, int capacity, const float* emitters,
                             int emit_capacity, void* scratch, float* out, hipStream_t s);

// fft4k.hip (N = 2048, 4096: pass_c4_supported): four-step column passes C1 (in place on the
// 16-wide tile-major intermediate) + C2 (with the pass-B epilogue); replace pass B.
hipError_t launch_pass_c4(const DevView& v, hipStream_t s);
// Mirror-pair row pass (N = 512 / 1024, 4 planes): one item = rows y and N - y; the
// texels k and -k share wave data and the phase factor and read h0 once (h0k).  Sizes: frame_plan.h pass_a4_supported.
hipError_t launch_pass_a_v4(const DevView& v, float t, hipStream_t s);
// fftq.hip: the fused frame through a three-plane intermediate (full outputs): pass AQ
// (mirror-pair rows, N = 512 / 1024) or A3Q (one row per item, N = 2048 / 4096), then pass BQ
// (column tiles, four transforms, N <= 1024) or the four-step column passes with Q planes.  Sizes: pass_q_supported.
// Band-limited cascades (N = 512 / 1024, full column band): the live rows of a view's units, device
// pointers.  tab = the view's `items` live items of pass AQ, each (context unit << 16 | y1) with the
// view's unit 0 being context unit ubase (prune_items.h); ext = the live extent m_u of each unit of the
// view (launch_live_extent).  Pass AQ then writes live rows only and pass BQ loads live rows only, so
// both passes of a chunk take the same PruneView or none (null: the dense schedule).
struct PruneView {
    const int* tab;
    int items;
    int ubase;
    const int* ext;
};
hipError_t launch_pass_a_q(const DevView& v, float t, hipStream_t s, const PruneView* pv = nullptr);
hipError_t launch_pass_b_q(const DevView& v, hipStream_t s, const PruneView* pv = nullptr);
// fft4k.hip with the three-plane intermediate: C1 also forms and transforms R[Q4] into the fourth
// plane slot; C2 runs the three-plane epilogue.
hipError_t launch_pass_c4q(const DevView& v, hipStream_t s);

}  // namespace ocean
