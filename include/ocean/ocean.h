/*
 * ocean.h -- C ABI of liboceanhip.so, the MI355X (gfx950) implementation of the
 * reference's per-frame Tessendorf ocean path (Mozobo/Ocean-Simulation).
 *
 * The reference boundary is Unity's ComputeShader binding API driven from C#:
 * WaterBody.cs binds textures/buffers by string name and Dispatch()es the
 * InitialSpectrum / TimeDependentSpectrum / IFFT / ResultTexturesFiller kernels,
 * and the output stays in Tex2DArray RenderTextures read by Water.shader and by
 * AsyncGPUReadback (WaterBody.cs:180-193, :288-296).  Each entry point below
 * names the reference interface it replaces.  A C# P/Invoke binding of every
 * symbol is given in INTEGRATION.md.
 *
 * Conventions
 *   - cdecl, every struct blittable (LayoutKind.Sequential in C#).
 *   - Every int-returning call returns OCEAN_OK (0) or a negative OCEAN_E_*;
 *     no C++ exception crosses the ABI.  ocean_last_error() gives a
 *     thread-local message for the last failure on the calling thread.
 *   - The context owns all device memory; the caller owns host buffers, which
 *     are only read/written during the call.
 *   - GPU work is enqueued on the context's own HIP stream (one per ctx); only
 *     ocean_read / ocean_write / ocean_synchronize / ocean_set_noise /
 *     ocean_generate_noise block the calling thread.
 *   - A context is not thread-safe: drive it from one thread (like Unity's
 *     main thread).  Multi-GPU = one context per device.
 *   - The calling thread's current HIP device is never changed: a call makes
 *     its context's device current for the span of the call and restores the
 *     caller's device before it returns (ocean_create / ocean_destroy /
 *     ocean_readback_release included).  One thread may drive contexts on
 *     several devices, beside torch or any other HIP user, in any order.
 *
 * Memory layout in HBM (all fp32, texture index = [unit][y][x], unit = tile*C + cascade,
 * matching Unity's Tex2DArray [slice][y][x] with id.x = x):
 *   NOISE  float2 [T][N][N]       H0    float4 [T*C][N][N]   WAVES float4 [T*C][N][N]
 *   PLANEp float2 [T*C][N][N]     p = 0 DxDz, 1 DyDxz, 2 DyxDyz, 3 DxxDzz
 *   DISP   float4 [T*C][N][N]     DERIV float4 [T*C][N][N]  TURB  float4 [T*C][N][N]
 *   NORMAL float4 [T*C][N][N]     (derived output, OCEAN_F_NORMALS only)
 *   VEL    float4 [T*C][N][N]     (derived output, OCEAN_F_VELOCITY only; zero after ocean_create)
 */
#ifndef OCEAN_OCEAN_H
#define OCEAN_OCEAN_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Version history (a host checks ocean_abi_version() at load time):
 *   1  round-1 entry points.
 *   2  semantics changed: ocean_set_params only stages values until ocean_init_spectrum;
 *      ocean_init_spectrum no longer zeroes the foam (ocean_reset_foam does); ocean_write
 *      of OCEAN_TEX_WAVES is E_UNSUPPORTED without OCEAN_F_UNFUSED; ocean_sample_world*
 *      return E_STATE before ocean_init_spectrum and the device entry checks alignment.
 *      New: ocean_reset_foam, ocean_set_column_band, ocean_sample_world(_device),
 *      ocean_read_async family, ocean_host_alloc/free, ocean_generate_noise_device,
 *      ocean_kernel_name, ocean_set_column_parity.
 *   3  semantics changed: no call moves the calling thread's current HIP device any more
 *      (Conventions).  New: ocean_readback_copy_ms.
 *   4  semantics changed: ocean_readback_copy_ms needs a request made with readback timing on
 *      (ocean_set_readback_timing; off by default, so a host that never asks for copy times
 *      records no timing events).  New: ocean_read_height_async, ocean_set_readback_timing.
 *      Added within version 4, with no change to any existing entry: ocean_query_surface,
 *      ocean_query_surface_device, ocean_query_surface_async.  The version number does not tell
 *      a library that has them from one that does not: a host that needs them probes for the
 *      symbol (dlsym / EntryPointNotFoundException).
 *      Added later within version 4 in the same way: ocean_surface_grid, ocean_surface_grid_device,
 *      ocean_surface_grid_async.
 *      Added later within version 4 in the same way: ocean_body_buoyancy, ocean_body_buoyancy_device,
 *      ocean_body_buoyancy_async.
 *      Added later within version 4 in the same way: OCEAN_F_VELOCITY, OCEAN_TEX_VELOCITY, ocean_query_velocity,
 *      ocean_query_velocity_device, ocean_query_velocity_async.
 *      Added later within version 4 in the same way: ocean_surface_bounds, ocean_surface_bounds_device,
 *      ocean_raycast, ocean_raycast_device, ocean_raycast_async.
 *      Added later within version 4 in the same way: OCEAN_DRAG_LINEAR, OCEAN_DRAG_QUADRATIC, ocean_body_dynamics,
 *      ocean_body_dynamics_device, ocean_body_dynamics_async.
 *      Added later within version 4 in the same way: OCEAN_WHITECAP_MAX_RECORDS, ocean_whitecaps,
 *      ocean_whitecaps_device, ocean_whitecaps_async.
 *      Added later within version 4 in the same way: OCEAN_CAMERA_HITS, OCEAN_CAMERA_RANGE, OCEAN_CAMERA_COLOR,
 *      ocean_camera, ocean_camera_device, ocean_camera_async.
 *      Added later within version 4 in the same way: OCEAN_BODY_STEP_FLOATS, OCEAN_BODY_MAX_SUBSTEPS,
 *      OCEAN_BODY_STEP_MAX_SAMPLES, ocean_body_step, ocean_body_step_device, ocean_body_step_async.
 *      Added later within version 4 in the same way: OCEAN_ATMOSPHERE_FLOATS, OCEAN_ATMOSPHERE_MAX_DIM, OCEAN_LUT_*,
 *      OCEAN_CAMERA_SKY_LUT, ocean_atmosphere, ocean_sky_update, ocean_atmosphere_read, ocean_atmosphere_lut,
 *      ocean_sun_color.
 *      Added later within version 4 in the same way: OCEAN_SPRAY_FLOATS, OCEAN_SPRAY_MAX_PARTICLES,
 *      OCEAN_SPRAY_MAX_STAGED, OCEAN_SPRAY_MAX_SUBSTEPS, ocean_spray_step, ocean_spray_step_device,
 *      ocean_spray_step_async.
 *      Added later within version 4 in the same way: OCEAN_RAY_BODY, OCEAN_BODY_PAINT_FLOATS, ocean_camera_bodies,
 *      ocean_camera_bodies_device, ocean_camera_bodies_async.
 *      Added later within version 4 in the same way: OCEAN_CAMERA_LINKS, OCEAN_SCENE_OPTICS_FLOATS, ocean_camera_scene,
 *      ocean_camera_scene_device, ocean_camera_scene_async.
 *      Added later within version 4 in the same way: OCEAN_HULL_MAX_VERTICES, OCEAN_HULL_MAX_TRIANGLES,
 *      OCEAN_HULL_RECORD_FLOATS, ocean_body_hydrostatics, ocean_body_hydrostatics_device,
 *      ocean_body_hydrostatics_async. */
#define OCEAN_ABI_VERSION 4

/* status codes */
#define OCEAN_OK 0
#define OCEAN_E_INVALID_ARG (-1)   /* bad pointer, size, index or enum */
#define OCEAN_E_UNSUPPORTED (-2)   /* N not a power of two in [16, 4096], C not in [1, 5], ... */
#define OCEAN_E_STATE (-3)         /* call order violated (e.g. step before init_spectrum) */
#define OCEAN_E_DEVICE (-4)        /* HIP runtime / kernel launch failure */
#define OCEAN_E_OUT_OF_MEMORY (-5) /* hipMalloc failed */

/* ocean_create flags */
#define OCEAN_F_DISPLACEMENT_ONLY 0x1u /* 2 planes (DxDz, DyDxz) -> DISP only (BASELINE cfg2) */
#define OCEAN_F_NORMALS 0x2u           /* also write the per-cascade NORMAL texture (Water.shader:346-348) */
#define OCEAN_F_UNFUSED 0x4u           /* ocean_step runs the reference-shaped schedule:
                                          evolve -> 4 x ifft2d -> fill (WaterBody.cs:180-190) */
#define OCEAN_F_MIPS 0x8u              /* allocate mip chains for DERIV and TURB and regenerate them
                                          in every ocean_step (WaterBody.cs:191-192, :228-229) */
#define OCEAN_F_VELOCITY 0x10u         /* also keep the VELOCITY texture, the time derivative of DISP, written
                                          by every ocean_step (see ocean_query_velocity); combines with every
                                          other flag */

/* texture ids for ocean_read / ocean_read_async / ocean_write / ocean_get_device_ptr */
enum ocean_texture {
    OCEAN_TEX_NOISE = 0,  /* _RandomNoiseTexture           WaterBody.cs:86-100 (per tile, cascade ignored) */
    OCEAN_TEX_H0 = 1,     /* _InitialSpectrumTextures      InitialSpectrum.compute:14 */
    OCEAN_TEX_WAVES = 2,  /* _WavesDataTextures            InitialSpectrum.compute:15 */
    OCEAN_TEX_PLANE0 = 3, /* _DxDzTextures                 TimeDependentSpectrum.compute:6 */
    OCEAN_TEX_PLANE1 = 4, /* _DyDxzTextures */
    OCEAN_TEX_PLANE2 = 5, /* _DyxDyzTextures */
    OCEAN_TEX_PLANE3 = 6, /* _DxxDzzTextures */
    OCEAN_TEX_DISP = 7,   /* _DisplacementsTextures        ResultTexturesFiller.compute:7 */
    OCEAN_TEX_DERIV = 8,  /* _DerivativesTextures          ResultTexturesFiller.compute:8 */
    OCEAN_TEX_TURB = 9,   /* _TurbulenceTextures (foam state) ResultTexturesFiller.compute:9; the array may be
                             written on demand from the 4-byte state (ocean_step, "Deferred TURB") */
    OCEAN_TEX_NORMAL = 10, /* derived: normalize(-Dyx/(1+Dxx), 1, -Dyz/(1+Dzz)), w = 0 */
    OCEAN_TEX_VELOCITY = 11 /* derived: d/dt of DISP.xyz, and dDxz/dt in .w (OCEAN_F_VELOCITY only;
                               E_INVALID_ARG on any other context; written like OCEAN_TEX_NORMAL) */
};

typedef struct ocean_ctx ocean_ctx;

/* WaterBody public ocean parameters, WaterBody.cs:10-14. */
typedef struct ocean_params {
    float wind_speed;
    float wind_dir_x;
    float wind_dir_y;
    float gravity;
    float fetch;
    float depth;
} ocean_params;

/* WaterCascade component, WaterCascade.cs:10-24 (flattened as WaterBody.cs:231-242). */
typedef struct ocean_cascade {
    float wavelength; /* patch length L */
    float cutoff_low;
    float cutoff_high;
    float swell;
    float fade;
} ocean_cascade;

/* Replaces WaterBody.Awake resource creation (WaterBody.cs:211-251) and
 * new IFFT(...) (IFFT.cs:24-62): allocates every texture for `n_tiles`
 * independent oceans of `n_cascades` cascades at N = `n` on HIP device
 * `device`, and builds the twiddle table.  16 <= n <= 4096, power of two;
 * 1 <= n_cascades <= 5 (Water.shader:139); n_tiles >= 1. */
int ocean_create(int device, int n, int n_cascades, int n_tiles, uint32_t flags, ocean_ctx **out);

/* Replaces OnDisable (WaterBody.cs:300-309) + RT release.  NULL is a no-op. */
void ocean_destroy(ocean_ctx *ctx);

/* Replaces the SetFloat/SetBuffer parameter bindings of
 * InitializeInitialSpectrumComputeShader (WaterBody.cs:130-148).
 * `cascades` has n_cascades entries.  The values are only staged: they take effect
 * at the next ocean_init_spectrum, and frames stepped before it keep running with
 * the previous spectrum's constants (fused and unfused alike). */
int ocean_set_params(ocean_ctx *ctx, const ocean_params *params, const ocean_cascade *cascades);

/* Replaces GenerateRandomNoiseTexture + Texture2D.Apply (WaterBody.cs:86-100, :97):
 * uploads tile `tile`'s noise, float2[N][N] laid out [y][x] (g1, g2). Blocking. */
int ocean_set_noise(ocean_ctx *ctx, int tile, const float *rg);

/* This library's documented, seeded noise (the reference's UnityEngine.Random is
 * unseeded and closed): tile t uses seed + t; Marsaglia polar over xorshift128
 * seeded by splitmix64, texels generated x-outer / y-inner, g1 then g2
 * (WaterBody.cs:71-100).  Generated on the host, uploaded.  Blocking. */
int ocean_generate_noise(ocean_ctx *ctx, uint64_t seed);

/* On-device noise for large tile batches (replaces the CPU
 * loop of WaterBody.cs:86-100): a counter-based generator, one independent stream
 * per texel -- a different sequence from ocean_generate_noise.  Texel (x, y) of
 * tile t: key = mix(seed + t + G) ^ ((y*N + x) * 0xD1B54A32D192ED03), uniform k
 * (k = 1, 2, ...) = (mix(key + k*G) >> 40) * 2^-24 with G = 0x9E3779B97F4A7C15 and
 * mix the splitmix64 finaliser; g1 then g2 each from the Marsaglia polar loop
 * (WaterBody.cs:71-81).  Blocking. */
int ocean_generate_noise_device(ocean_ctx *ctx, uint64_t seed);

/* Replaces CalculateInitialSpectrumTextures (WaterBody.cs:171-178):
 * InitialSpectrum.compute:99-129 then :135-143 for every tile and cascade, with
 * the parameters staged by ocean_set_params.  The foam state (TURB) is left as it
 * is, as in the reference's re-init on a parameter change (the commented
 * OnValidate, WaterBody.cs:324-337); it is zero after ocean_create.  Blocks until
 * the staged constants are on the device, then runs async on the ctx stream. */
int ocean_init_spectrum(ocean_ctx *ctx);

/* Zeroes the foam accumulator (TURB, its mip chain and the internal foam state)
 * of every tile and cascade, stream-ordered.  No reference counterpart: there the
 * RenderTexture starts zeroed once (WaterBody.cs:229) and is never cleared. */
int ocean_reset_foam(ocean_ctx *ctx);

/* Replaces CalculateWavesTexturesAtTime(time) (WaterBody.cs:180-193, minus
 * GenerateMips): evolve -> 2D IFFT of every plane -> fill/foam for all tiles
 * and cascades.  Async on the ctx stream.  Fused 2-kernel schedule by default;
 * OCEAN_F_UNFUSED selects the reference-shaped one (same results to rounding).
 *
 * Deferred TURB.  TURB is (f, f, f, f) of the 4-byte foam state f the step keeps beside it, and every consumer
 * in this library reads .x alone.  A frame whose column passes are all pass BQ (N = 512 or 1024, full outputs,
 * h0 from ocean_init_spectrum, whole column band, fused schedule) therefore stores the foam state only: the
 * consumers of the finished textures (ocean_sample_world, the queries, grids, bodies, ray casts, whitecaps, spray,
 * cameras) tap the state as TURB's level 0, bit-identical to tapping the array, and OCEAN_F_MIPS chains are boxed
 * from the state as always.  The float4 array is written from the state, by one kernel of kind 2 on the ctx stream,
 * when an entry shows the array itself: ocean_read, ocean_read_mip level 0 and ocean_read_async of OCEAN_TEX_TURB,
 * ocean_write of it (before the upload, so that the other slices hold), ocean_set_column_band of a band narrower than N, and
 * ocean_get_device_ptr (below).  What these entries return is what a context that writes TURB every frame returns.
 * OCEAN_DEFER_TURB=0 makes every frame write the array. */
int ocean_step(ocean_ctx *ctx, float time);

/* Column band for splitting one (tile, cascade) unit over several GPUs (SURVEY.md 8e,
 * "units < GPUs", cfg5 = 4 cascades on 8 GPUs; no reference counterpart -- the
 * reference runs every unit on one GPU).  After this call ocean_step computes the
 * full row IFFT of every row (the rows are needed whole) but stores, column-transforms
 * and fills only the columns x_begin <= x < x_begin + x_count of every slice: DISP,
 * DERIV, TURB and NORMAL are written there, bit-identical to a whole-band context's
 * texels, and the other columns are left as they are (zero after ocean_create).
 * Two contexts with complementary bands (one per GPU) produce a cascade between them
 * with no data exchange.  x_begin and x_count are multiples of g = min(N, max(16,
 * 8192 / N)); (0, N) restores the whole band.  Needs the fused schedule (not
 * OCEAN_F_UNFUSED) and no OCEAN_F_MIPS; the unfused stages (ocean_evolve,
 * ocean_ifft2d, ocean_fill) ignore the band. */
int ocean_set_column_band(ocean_ctx *ctx, int x_begin, int x_count);

/* Column parity, the other way to split one unit over two GPUs (no reference
 * counterpart): with parity b in {0, 1} the context computes only the output columns x = 2m + b,
 * m < N/2, of every slice, by decimation in frequency of the row transform (each row is evolved
 * whole, folded to z_b[n] = (a[n] + (-1)^b a[n + N/2]) e^{2 pi i b n / N} and transformed at N/2
 * points), so the two ranks of a unit do not duplicate the row transform as column bands do.
 * Column x = 2m + b is stored COMPACT at texture column m (DISP, DERIV, TURB, NORMAL: the first
 * N/2 columns of each texture row; the rest are left as they are); the consumer interleaves the
 * two ranks' textures.  Results equal the whole context's within the fp32 tolerance (a different
 * radix order), not bit for bit.  N = 4096, fused full-output schedule, no OCEAN_F_MIPS; -1 turns
 * it off (whole band again).  ocean_set_column_band replaces a parity; world sampling of a parity
 * context returns OCEAN_E_UNSUPPORTED. */
int ocean_set_column_parity(ocean_ctx *ctx, int parity);

/* Replaces the TimeDependentSpectrum dispatch alone (WaterBody.cs:181-182;
 * TimeDependentSpectrum.compute:20-47): writes PLANE0..3 at `time`.  Async. */
int ocean_evolve(ocean_ctx *ctx, float time);

/* Replaces IFFT.InverseFastFourierTransform(RenderTexture) (IFFT.cs:66-94) for
 * every plane p with bit p set in `plane_mask`: in place,
 * out[m] = (-1)^(mx+my) * sum_{x,y} in[x,y] e^{+2 pi i (x mx + y my)/N}
 * over all tiles and cascades.  Async. */
int ocean_ifft2d(ocean_ctx *ctx, int plane_mask);

/* Replaces the FillResultTextures dispatch (WaterBody.cs:189;
 * ResultTexturesFiller.compute:16-34): PLANE0..3 + TURB -> DISP, DERIV, TURB.  Async. */
int ocean_fill(ocean_ctx *ctx);

/* Synchronous texture readback of one (tile, cascade) slice, replacing
 * AsyncGPUReadback.Request(...).GetData<Color>() (WaterBody.cs:288-296).
 * `bytes` must equal the slice size (N*N*16 for float4, N*N*8 for float2).
 * Orders after all work queued on the ctx stream. */
int ocean_read(ocean_ctx *ctx, int texture, int tile, int cascade, void *dst, size_t bytes);

/* Synchronous upload of one slice (foam state for resume, planes for
 * operator-level tests).  Same size rules as ocean_read.  OCEAN_TEX_WAVES is
 * writable only with OCEAN_F_UNFUSED (E_UNSUPPORTED otherwise): the fused row pass
 * rebuilds the wave data from the active parameters every frame. */
int ocean_write(ocean_ctx *ctx, int texture, int tile, int cascade, const void *src, size_t bytes);

/* Zero-copy access for same-process consumers: base device pointer and total
 * byte size of a texture (all tiles and cascades).
 * OCEAN_TEX_TURB: the call writes the array from the foam state if a deferred frame (ocean_step) has left it
 * stale, stream-ordered, and from then on every ocean_step of this context writes TURB, for the life of the
 * context: a reader through the pointer cannot be seen.  A renderer takes the pointer once, before its first
 * frame, and then runs the frames this library ran before TURB could be deferred. */
int ocean_get_device_ptr(ocean_ctx *ctx, int texture, void **ptr, size_t *bytes);

/* The ctx's hipStream_t (as void*), for callers that order their own work. */
int ocean_get_stream(ocean_ctx *ctx, void **stream);

/* Blocks until all work queued on the ctx stream has finished. */
int ocean_synchronize(ocean_ctx *ctx);

/* Kernel timing: when enabled, each kernel launch of ocean_step / ocean_ifft2d
 * is bracketed by HIP events on the ctx stream; ocean_kernel_stats returns, for
 * kernel `kind` (0 = pass A / row pass, 1 = pass B / column pass, 2 = other),
 * the summed duration in ms and the launch count since the last reset
 * (synchronizes the stream).  At most 2048 launches' events are held: past that
 * the finished ones are folded into the sums (waiting for the oldest if none
 * has finished), and disabling timing folds the rest, so a host that never
 * polls holds a bounded number of events. */
int ocean_set_kernel_timing(ocean_ctx *ctx, int enable);
int ocean_kernel_stats(ocean_ctx *ctx, int kind, double *total_ms, long long *launches);

/* Symbol (demangled, as rocprofv3 reports it) of the kernel most recently launched in `kind`
 * (0, 1, 2 as above) by this context, NUL-terminated into buf[len].  OCEAN_E_STATE if none yet;
 * OCEAN_E_INVALID_ARG if it does not fit.  Measurement only (no reference counterpart): lets a
 * bench match profiler records to the exact kernel that ran. */
int ocean_kernel_name(ocean_ctx *ctx, int kind, char *buf, size_t len);

/* Algorithmic HBM bytes one ocean_step moves in the schedule this context runs
 * (the roofline numerator; no reference counterpart -- measurement only):
 * fused: *pass_a = pass A (evolve + row IFFT), *pass_b = pass B (column IFFT +
 * fill); OCEAN_F_UNFUSED: *pass_a = evolve + row launches, *pass_b = column
 * launches + fill.  Depends on the kernels selected for N, the flags and the
 * state (e.g. after ocean_write(H0) pass A reads the full h0). */
int ocean_step_bytes(ocean_ctx *ctx, uint64_t *pass_a, uint64_t *pass_b);

/* Mip chains (OCEAN_F_MIPS), the GenerateMips of WaterBody.cs:191-192.  Level
 * L >= 1 of a slice is (N >> L)^2 RGBA fp32 texels, [y][x]; texel (x, y) =
 * ((a + b) + (c + d)) * 0.25 over the 2x2 texels (2x, 2y), (2x+1, 2y),
 * (2x, 2y+1), (2x+1, 2y+1) of level L-1 (a box filter: Unity's filter is not
 * specified).  Level 0 is the texture itself.  `texture` is OCEAN_TEX_DERIV or
 * OCEAN_TEX_TURB; bytes must equal (N >> level)^2 * 16.  Blocking, like ocean_read.
 * Device layout (ocean_get_mip_ptr): one chain per slice, levels 1..log2 N
 * concatenated, slice-major; *ptr points at level `level` of slice 0 and
 * *slice_stride is the distance in bytes between consecutive slices' chains. */
int ocean_read_mip(ocean_ctx *ctx, int texture, int tile, int cascade, int level, void *dst, size_t bytes);
int ocean_get_mip_ptr(ocean_ctx *ctx, int texture, int level, void **ptr, size_t *slice_stride);

/* Cascade-summed world sampling, the texture reads of the reference's consumer
 * (Water.shader:314-348).  Point i of `points` is (world x,
 * world z, lod) as float[3]; out[i] is float[12]:
 *   out[12i + 0..3]  = sum_c DISP_c(uv_c).xyz, sum_c (1 - saturate(TURB_c(uv_c, lod).x))
 *   out[12i + 4..7]  = sum_c DERIV_c(uv_c, lod)            (Dyx, Dyz, Dxx, Dzz)
 *   out[12i + 8..11] = normalize(-sx, 1, -sz), 0 with s = (d.x / (1 + d.z), d.y / (1 + d.w))
 * over the cascades c of tile `tile`, uv_c = (x, z) / L_c (L_c = the active cascade
 * wavelength), summed in cascade order from 0.  Filtering (this library's definition;
 * Unity's RenderTextures are Repeat-wrapped and trilinear, WaterBody.cs:112-113):
 * on an m x m level, s = uv * m - 0.5, texels floor(s) and floor(s) + 1 mod m, weights
 * f = s - floor(s), lerp(a, b, f) = a + f (b - a), x first then y.  DISP has no mips
 * (WaterBody.cs:227) and is read at level 0; DERIV and TURB blend levels floor(lod)
 * and floor(lod) + 1 (lod clamped to [0, log2 N]) when the context has OCEAN_F_MIPS,
 * else level 0.  DISPLACEMENT_ONLY contexts return zero derivatives and turbulence.
 * ocean_sample_world takes host buffers and blocks; ocean_sample_world_device takes
 * device pointers (points 4-B aligned, out 16-B aligned, else OCEAN_E_INVALID_ARG) and
 * is async on the ctx stream, ordered after the queued steps.  count = 0 is a no-op.
 * Both return OCEAN_E_STATE before ocean_init_spectrum. */
int ocean_sample_world(ocean_ctx *ctx, int tile, const float *points, int count, float *out);
int ocean_sample_world_device(ocean_ctx *ctx, int tile, const float *points, int count, float *out);

/* Asynchronous readback, the AsyncGPUReadback.Request(tex, 0, callback) of
 * WaterBody.cs:288-296: copies one slice (level 0) to `dst` on a copy stream once
 * the work queued so far on the ctx stream (e.g. the last ocean_step) has finished,
 * without blocking the caller.  `dst` must stay valid until the request is done;
 * for a truly asynchronous copy it should come from ocean_host_alloc (pinned).
 * ocean_readback_status: 1 done, 0 pending, < 0 error (the request's hasError).
 * ocean_readback_wait blocks until done.  Every request is freed with
 * ocean_readback_release (after completion; releasing a pending request waits). */
typedef struct ocean_readback ocean_readback;
int ocean_read_async(ocean_ctx *ctx, int texture, int tile, int cascade, void *dst, size_t bytes,
                     ocean_readback **out);
int ocean_readback_status(ocean_readback *rb);
int ocean_readback_wait(ocean_readback *rb);
void ocean_readback_release(ocean_readback *rb);
/* Height-only readback for buoyancy: the reference reads displacement slice 0 back every frame
 * (WaterBody.cs:288-296) into its private buoyancyData (:58), whose only reader, GetWaterHeight,
 * returns the .g channel alone (:195-209).  This request copies just that channel, DISP.y = Dy of one
 * (tile, cascade) slice, as float[N][N] laid out [y][x] (`bytes` = N*N*4: a quarter of the RGBA
 * slice over the link), with ocean_read_async's snapshot and completion semantics: the same
 * ocean_readback_status / _wait / _release / _copy_ms apply.  dst[y*N + x] is bit-identical to
 * the .y of texel (x, y) of the RGBA slice read at the same point of the stream. */
int ocean_read_height_async(ocean_ctx *ctx, int tile, int cascade, float *dst, size_t bytes,
                            ocean_readback **out);

/* Surface queries: the point lookups of a buoyancy consumer done on the device, so that a host
 * with M bodies moves M x 32 B per frame instead of a displacement slice (the reference reads
 * slice 0 back every frame, WaterBody.cs:288-296, only for GetWaterHeight, :195-209, which
 * BuoyantObject.FixedUpdate calls once per body).  Point i of `points` is (world x, world z) as
 * float[2]; out[i] is float[8].  With S(p) = what ocean_sample_world returns for the point
 * (p.x, p.z, lod 0) of tile `tile` (DERIV and TURB at level 0 also on OCEAN_F_MIPS contexts):
 *
 *   OCEAN_QUERY_SURFACE, iterations = K in [0, 16]: the height of the surface ABOVE q = (x, z).
 *   The displacement is Lagrangian (the grid point p lands at p + D_xz(p)), so the water over q is
 *   Dy(p*) with p* + D_xz(p*) = q; K steps of that fixed point, all in fp32 in this order:
 *       p_0 = q;  for k < K:  D = S(p_k)[0..2],  p_{k+1} = (q.x - D.x, q.z - D.z);  D = S(p_K)[0..2]
 *       out[8i + 0..3] = D.y, p_K.x, p_K.z, r = max(|(p_K.x + D.x) - q.x|, |(p_K.z + D.z) - q.z|)
 *       out[8i + 4..7] = S(p_K)[8..10] (the normal at p_K), S(p_K)[3] (the foam at p_K)
 *   r is the distance by which p_K misses q, i.e. the length of the step K + 1 would take.  The
 *   iteration contracts where the displacement's Lipschitz constant is below 1 (no folded,
 *   self-intersecting surface); elsewhere it stays bounded (|p_k - q| <= max |D_xz|) and r says so.
 *   K = 0 is ocean_sample_world at q.  DISPLACEMENT_ONLY contexts give the normal (0, 1, 0), foam 0.
 *
 *   OCEAN_QUERY_REFERENCE, iterations = 0: GetWaterHeight's own texel pick (WaterBody.cs:195-209)
 *   in fp32: a = -(N/2), b = N/2, u = saturate((x - a) / (b - a)), px = clamp((int)(u N), 0, N - 1),
 *   py alike from z;  out[8i + 0..7] = DISP[tile * C + 0][py][px].y, (float)px, (float)py, 0, 0, 0, 0, 0
 *   (cascade 0 of the tile, as the reference's slice 0).
 *
 * ocean_query_surface takes host buffers and blocks.  ocean_query_surface_device takes device
 * pointers (points 4-B aligned, out 16-B aligned, else OCEAN_E_INVALID_ARG; any count >= 0) and is
 * async on the ctx stream, ordered after the queued steps.  ocean_query_surface_async is the
 * per-frame form: `points` is a host buffer consumed before the call returns (the caller may reuse
 * it at once); the query runs on the ctx stream, after the steps queued so far and before later
 * ones, and its count x 32 B land in `dst` on the copy stream like an ocean_read_async slice, with
 * the same ocean_readback_status / _wait / _release / _copy_ms.
 * All three: OCEAN_E_INVALID_ARG for a null pointer, count < 0, count > OCEAN_QUERY_MAX_POINTS (host
 * and async forms), an unknown mode, iterations outside [0, 16] or nonzero in reference mode, or a
 * tile out of range, all checked before any device call; then OCEAN_E_STATE before
 * ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context (as world sampling).
 * count = 0 is a no-op in the blocking and device forms and OCEAN_E_INVALID_ARG in the async form
 * (there is no request to hand back). */
#define OCEAN_QUERY_REFERENCE 0
#define OCEAN_QUERY_SURFACE 1
#define OCEAN_QUERY_MAX_POINTS 65536
int ocean_query_surface(ocean_ctx *ctx, int tile, int mode, int iterations, const float *points, int count,
                        float *out);
int ocean_query_surface_device(ocean_ctx *ctx, int tile, int mode, int iterations, const float *points, int count,
                               float *out);
int ocean_query_surface_async(ocean_ctx *ctx, int tile, int mode, int iterations, const float *points, int count,
                              float *dst, ocean_readback **out);

/* Surface grids: the surface over the nodes of a regular grid, for the consumers that read it over an
 * area and not at scattered points.  The reference's renderer builds a regular plane
 * (MeshGenerator.cs:19-35: planeSize / trianglesSize cells a side, 101 x 101 vertices by default) and
 * the domain stage of Water.shader (:314-334) moves every vertex by the cascade-summed displacement at
 * its world position; a heightfield collider, a top-down map or a shoreline pass wants the height above
 * every node.  No point list is passed: the grid is six numbers, (x0, z0, dx, dz, nx, ny).  Node (i, j),
 * i < nx along world x and j < ny along world z, lies at
 *       q.x = x0 + (float)i * dx,   q.z = z0 + (float)j * dz     (one fp32 multiply and one fp32 add each)
 * and its result is element k = j * nx + i of `out`.  Zero and negative spacings are valid.  With S(p)
 * what ocean_sample_world returns for the point (p.x, p.z, lod) of tile `tile`:
 *
 *   OCEAN_GRID_VERTICES, iterations = 0, lod >= 0: the displaced mesh of the domain stage.
 *       out[8k + 0..3] = q.x + S(q)[0], S(q)[1], q.z + S(q)[2], S(q)[3]   (the vertex, fp32 adds; the foam)
 *       out[8k + 4..7] = S(q)[8..11]                                      (the normal, 0)
 *   DERIV and TURB use `lod` exactly as ocean_sample_world does (trilinear on OCEAN_F_MIPS contexts,
 *   level 0 otherwise); DISP is always read at level 0.
 *
 *   OCEAN_GRID_SURFACE, iterations = K in [0, 16], lod = 0: the Eulerian surface.  out[8k + 0..7] is the
 *   8-float record of OCEAN_QUERY_SURFACE for the point q with K iterations, bit for bit.
 *
 *   OCEAN_GRID_HEIGHTFIELD, same arguments: element 0 of that record alone, float[ny][nx]: 4 B per node
 *   for colliders and readbacks.
 *
 * `bytes` must equal nx * ny * 32 (vertices, surface) or nx * ny * 4 (heightfield).
 * ocean_surface_grid: `out` is a host buffer; blocks, as ocean_query_surface.
 * ocean_surface_grid_device: `out` is a device pointer, 16-B aligned in every mode (else
 * OCEAN_E_INVALID_ARG); async on the ctx stream, ordered after the queued steps: a renderer's vertex
 * buffer is filled with no host copy.
 * ocean_surface_grid_async: `out` is a host destination (pinned, ocean_host_alloc, for a truly
 * asynchronous copy).  The grid is computed into a readback slot on the ctx stream, after the steps
 * queued so far and before later ones, and copied on the copy stream like an ocean_read_async slice,
 * with the same ocean_readback_status / _wait / _release / _copy_ms.  The result must fit a slot:
 * bytes <= max(N * N * 16, OCEAN_QUERY_MAX_POINTS * 40), else OCEAN_E_INVALID_ARG.  *req is NULL after
 * every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null context, a null `out` or
 * `req`, a tile out of range, an unknown mode, iterations outside [0, 16] or nonzero in vertices mode,
 * a lod that is not finite, negative, or nonzero in surface and heightfield mode, a non-finite x0, z0,
 * dx or dz, nx < 1 or ny < 1, nx * ny > OCEAN_GRID_MAX_NODES (in 64 bits) or a wrong `bytes`; then
 * OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context (as the
 * queries). */
#define OCEAN_GRID_VERTICES 0
#define OCEAN_GRID_SURFACE 1
#define OCEAN_GRID_HEIGHTFIELD 2
#define OCEAN_GRID_MAX_NODES (1 << 22)
int ocean_surface_grid(ocean_ctx *ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                       float dx, float dz, int nx, int ny, float *out, size_t bytes);
int ocean_surface_grid_device(ocean_ctx *ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                              float dx, float dz, int nx, int ny, float *out, size_t bytes);
int ocean_surface_grid_async(ocean_ctx *ctx, int tile, int mode, int iterations, float lod, float x0, float z0,
                             float dx, float dz, int nx, int ny, float *out, size_t bytes, ocean_readback **req);

/* Buoyant bodies: M rigid bodies that share one hull of P probes, reduced on the device to 32 B per
 * body, whatever P is.  The reference's model is one probe per body with the volume from
 * transform.localScale (BuoyantObject.FixedUpdate -> GetWaterHeight; its README: "very basic"); a host
 * that wants hulls that roll and pitch puts P probes on each body, and with the queries above it would
 * transform M x P probes on the CPU, upload M x P x 8 B, read back M x P x 32 B and reduce them itself.
 * Here the transform, the surface lookup and the reduction are one kernel.
 *
 *   hull:   probe j is float[5] = (rx, ry, rz, h, v): the centre of the probe's cell in the body frame, the
 *           cell's vertical extent and its volume.
 *   bodies: body b is float[10] = (cx, cy, cz, qx, qy, qz, qw, sx, sy, sz): the world position of the body
 *           origin, a body -> world quaternion (the caller keeps it unit) and a per-axis scale (the role
 *           of the reference's transform.localScale).
 *   out:    record b is float[8].
 *
 * All arithmetic is fp32, each line one rounding per operation in the order written (no fused
 * multiply-add).  Per probe j of body b, with c = (cx, cy, cz), u = (qx, qy, qz), s = (sx, sy, sz):
 *       a   = (sx * rx, sy * ry, sz * rz)
 *       t   = 2 * (u x a),  (u x a) = (u.y * a.z - u.z * a.y,  u.z * a.x - u.x * a.z,  u.x * a.y - u.y * a.x)
 *       d   = (a + qw * t) + (u x t), componentwise, (u x t) formed like (u x a)        (a rotated by q)
 *       w   = c + d                                                                    (world position)
 *       mode OCEAN_QUERY_SURFACE, iterations = K in [0, 16]: rec = the 8-float record of ocean_query_surface
 *           for the point (w.x, w.z) with K iterations, bit for bit: eta = rec[0], r = rec[3], n = rec[4..6]
 *       mode OCEAN_QUERY_REFERENCE, iterations = 0: eta = rec[0] of that mode (GetWaterHeight's texel pick
 *           at (w.x, w.z)), n = (0, 1, 0), r = 0
 *       h'  = h * sy,   v' = ((v * sx) * sy) * sz                                      (the scaled cell)
 *       bottom = w.y - 0.5f * h',   f = fminf(fmaxf((eta - bottom) / h', 0), 1)        (submerged fraction)
 *       g   = v' * f                                                                   (submerged volume)
 *       e   = (d.x, (d.y - 0.5f * h') + 0.5f * (f * h'), d.z)       (centroid of the submerged part of the
 *                                                                    cell, relative to the body origin)
 *       the seven terms: g, g * e.x, g * e.y, g * e.z, g * n.x, g * n.y, g * n.z
 * The sum over a body's probes is defined exactly.  W = the smallest power of two >= P, capped at 64.
 * Lane l < W accumulates t_l from +0: t_l = t_l + term, for its probes j = l, l + W, l + 2W, ... in
 * ascending order; a lane without a probe keeps +0.  Then for s = W/2, W/4, ..., 1: t_l = t_l + t_(l xor s)
 * for every l.  The result is t_0 (in numpy: fold the upper half of t onto the lower half until one is left).
 *       out[8b + 0..6] = the seven sums
 *       out[8b + 7]    = fmaxf over the body's probes of r (the worst fixed-point residual, as in the queries)
 * What a host does with a record: the buoyant force is rho g out[0] along +y and acts at c + out[1..3] /
 * out[0]; its torque about c is rho g (-out[3], 0, out[1]); out[4..6] normalised is the water plane under
 * the hull.  The reference's box is approximately the one-probe hull (0, 0.5, 0, 1, 1) with the identity
 * quaternion in reference mode: its bottom at pos.y, its height localScale.y, its volume the product of
 * the scales.
 * The library does not inspect hull or body values: a non-unit quaternion scales and shears as the
 * formulas say, and h * sy = 0 or a non-finite input gives unspecified numbers (never an access outside
 * the textures).
 *
 * ocean_body_buoyancy takes host buffers and blocks.  ocean_body_buoyancy_device takes device pointers
 * (hull and bodies 4-B aligned, out 16-B aligned, else OCEAN_E_INVALID_ARG) and is async on the ctx
 * stream, ordered after the queued steps; count is bounded by OCEAN_BODY_MAX_SAMPLES alone.
 * ocean_body_buoyancy_async is the per-frame form, exactly as ocean_query_surface_async: `hull` and
 * `bodies` are host buffers consumed before the call returns; the kernel runs on the ctx stream, after
 * the steps queued so far and before later ones, and its count x 32 B land in `out` on the copy stream
 * like an ocean_read_async slice, with the same ocean_readback_status / _wait / _release / _copy_ms.
 * *req is NULL after every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null ctx, hull, bodies, out or
 * req, a tile out of range, an unknown mode, iterations outside [0, 16] or nonzero in reference mode,
 * probes outside [1, OCEAN_BODY_MAX_PROBES], count < 0, count > OCEAN_BODY_MAX_BODIES (host and async
 * forms, which stage the bodies), count * probes > OCEAN_BODY_MAX_SAMPLES (in 64 bits) or a misaligned
 * device pointer; then OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a
 * column-parity context (as the queries).  count = 0 is a no-op in the blocking and device forms and
 * OCEAN_E_INVALID_ARG in the async form (there is no request to hand back). */
#define OCEAN_BODY_MAX_BODIES 8192
#define OCEAN_BODY_MAX_PROBES 4096
#define OCEAN_BODY_MAX_SAMPLES (1 << 22)
int ocean_body_buoyancy(ocean_ctx *ctx, int tile, int mode, int iterations, const float *hull, int probes,
                        const float *bodies, int count, float *out);
int ocean_body_buoyancy_device(ocean_ctx *ctx, int tile, int mode, int iterations, const float *hull, int probes,
                               const float *bodies, int count, float *out);
int ocean_body_buoyancy_async(ocean_ctx *ctx, int tile, int mode, int iterations, const float *hull, int probes,
                              const float *bodies, int count, float *out, ocean_readback **req);

/* Surface velocity: how the water moves, where the entries above say where it is.  The reference's only
 * physics consumer applies drag against still water (BuoyantObject.FixedUpdate: -rb.velocity * drag); a host
 * that wants a hull to surge with a crest, drift down-wave or be damped relative to the water that carries
 * it, or that spawns spray and advects foam particles, needs the water's own velocity.  It is the inverse
 * transform of dh/dt, exact in t (no second frame, no difference of two readbacks).
 *
 * A context created with OCEAN_F_VELOCITY owns the texture OCEAN_TEX_VELOCITY, VEL float4 [T*C][N][N], zero
 * after ocean_create, and every ocean_step(t) writes it after the frame (and the mip chains), on the ctx
 * stream, under the fused and the OCEAN_F_UNFUSED schedule alike; DISPLACEMENT_ONLY contexts are supported
 * (only H0 and WAVES are read).  Without the flag a context allocates, launches and returns what it always
 * did.  All arithmetic is fp32, one rounding per operation in the order written (no fused multiply-add).
 * Per texel i, with h0 = H0[i], w = WAVES[i] (w.w = omega) and (ex, ey) = (cos, sin)(omega * t), the frame's
 * own phase factor (TimeDependentSpectrum.compute:25):
 *       A  = (h0.x * ex - h0.y * ey,     h0.x * ey + h0.y * ex)                (the two products of h(k, t), :26)
 *       B  = (h0.z * ex - h0.w * (-ey),  h0.z * (-ey) + h0.w * ex)
 *       g  = (A.x - B.x, A.y - B.y)
 *       ht = (-(g.y * w.w), g.x * w.w)                                         (dh/dt = i omega (A - B))
 *       V0, V1 = the DxDz and DyDxz packing of TimeDependentSpectrum.compute:27-43 applied to ht in place of h:
 *            ih = (-ht.y, ht.x);  dx = (ih * w.x) * w.y;  dz = (ih * w.z) * w.y;  aux = (-ht) * w.y;
 *            dzdx = (aux * w.x) * w.z;   V0 = (dx.x - dz.y, dx.y + dz.x);   V1 = (ht.x - dzdx.y, ht.y + dzdx.x)
 * Both planes go through the operator of ocean_ifft2d (centred, unnormalised, permuted), exactly as it
 * treats PLANE0 and PLANE1, and VEL[i] = (Re V0, Re V1, Im V0, Im V1).  Out-of-band texels (omega = 0) are zero.
 * The packing is the reference's on purpose: its spectrum is not Hermitian on the Nyquist row and column,
 * so DISP.y carries a leak of Dxz; with the same packing VEL.xyz is the exact time derivative of DISP.xyz as
 * this library computes it, that quirk included, and VEL.w is dDxz/dt, which the packing yields with it.
 * ocean_set_column_band with anything but the whole band, and ocean_set_column_parity with anything but
 * -1, return OCEAN_E_UNSUPPORTED on a velocity context.  The velocity launches count as kind 2 of
 * ocean_kernel_stats / ocean_kernel_name; kinds 0 and 1 and ocean_step_bytes keep meaning the frame's passes.
 *
 * ocean_query_velocity: point i of `points` is the world position q = (x, z) as float[2]; out[i] is float[8].
 * K = `iterations` in [0, 16] steps of ocean_query_surface's fixed point, the identical operations, then
 *       Vs(p) = sum over the cascades c, in order from 0, of VEL_c bilinearly filtered at (p.x / L_c, p.z / L_c)
 *               (level 0; the taps and the sum of ocean_sample_world's DISP)
 *       D = S(p_K)[0..2]
 *       out[8i + 0..3] = Vs(p_K).x, Vs(p_K).y, Vs(p_K).z, r        (r as in ocean_query_surface)
 *       out[8i + 4..7] = D.y, p_K.x, p_K.z, Vs(p_K).w
 * This is the velocity of the water PARTICLE that is on the surface above q: what drag and advection need.
 * It is not d eta / dt at the fixed position q; that is Vy - grad eta . V_xz, which a host forms from this
 * record and the normal of ocean_query_surface (grad eta = (-n.x / n.y, -n.z / n.y)).  K = 0 is the plain
 * cascade-summed sample of VEL at q.  Before the first ocean_step VEL is zero and the query is valid.
 * The three forms, their validation, limits, alignment, ordering, count = 0 and *req = NULL after every
 * failure are exactly those of ocean_query_surface, ocean_query_surface_device and ocean_query_surface_async
 * in OCEAN_QUERY_SURFACE mode (there is no mode argument): OCEAN_E_INVALID_ARG before any device call, then
 * OCEAN_E_UNSUPPORTED on a context without OCEAN_F_VELOCITY, OCEAN_E_STATE before ocean_init_spectrum and
 * OCEAN_E_UNSUPPORTED on a column-parity context.  The async form stages its points and lands count x 32 B
 * through the same readback slots. */
int ocean_query_velocity(ocean_ctx *ctx, int tile, int iterations, const float *points, int count, float *out);
int ocean_query_velocity_device(ocean_ctx *ctx, int tile, int iterations, const float *points, int count,
                                float *out);
int ocean_query_velocity_async(ocean_ctx *ctx, int tile, int iterations, const float *points, int count,
                               float *dst, ocean_readback **req);

/* Body dynamics: ocean_body_buoyancy with the drag against the water's own velocity beside it, reduced on the
 * device to 64 B per body, whatever P is.  The reference drags against still water (BuoyantObject.FixedUpdate:
 * -rb.velocity * drag); a host that damps a hull against the water that carries it (surge with a crest, drift
 * down-wave, roll damping) would, with the entries above, transform M x P probes on the CPU, upload them, read
 * M x P x 32 B of ocean_query_velocity back, form the relative velocity at every probe and reduce it itself.
 * Quadratic drag is not linear in a probe's relative velocity, so no per-body sum of the other entries yields it.
 * Needs a context created with OCEAN_F_VELOCITY.
 *
 *   hull:   float[P][5], exactly as ocean_body_buoyancy takes it.
 *   bodies: float[M][10], exactly as ocean_body_buoyancy takes it.
 *   motion: body b is float[6] = (vx, vy, vz, ox, oy, oz): the world-frame linear velocity of the body origin
 *           and the world-frame angular velocity (rad/s).
 *   out:    record b is float[16].
 *
 * All arithmetic is fp32, each line one rounding per operation in the order written (no fused multiply-add);
 * sqrtf and / are correctly rounded.  Per probe j of body b: a, t, d, w, h', v', rec, eta, r, n, f, g and e are
 * exactly as ocean_body_buoyancy defines them, and p_K = rec[1..2] is the point the fixed point ends on.  Then
 *       mode OCEAN_QUERY_SURFACE:   Vs = ocean_query_velocity's Vs(p_K)   (cascade-summed bilinear VEL at p_K: the
 *                                                                          same taps in the same order)
 *       mode OCEAN_QUERY_REFERENCE: Vs = VEL[tile * C + 0][py][px]        (the texel GetWaterHeight's pick chose,
 *                                                                          cascade 0)
 *       vb  = (vx + (oy * e.z - oz * e.y),  vy + (oz * e.x - ox * e.z),  vz + (ox * e.y - oy * e.x))
 *                                                                         (the body's velocity at the point e)
 *       u   = (Vs.x - vb.x, Vs.y - vb.y, Vs.z - vb.z)                     (the water relative to the hull)
 *       m   = sqrtf((u.x * u.x + u.y * u.y) + u.z * u.z)
 *       s   = g           (law OCEAN_DRAG_LINEAR)
 *       s   = g * m       (law OCEAN_DRAG_QUADRATIC)
 *       F   = (s * u.x, s * u.y, s * u.z)
 *       T   = (e.y * F.z - e.z * F.y,  e.z * F.x - e.x * F.z,  e.x * F.y - e.y * F.x)
 *       wet = f > 0 ? 1.0f : 0.0f
 * The fourteen summed terms are the seven of ocean_body_buoyancy, then F.x, F.y, F.z, T.x, T.y, T.z, wet, each
 * summed exactly as ocean_body_buoyancy sums: W lanes (the smallest power of two >= P, capped at 64), lane l
 * accumulating from +0 over j = l, l + W, ... in ascending order, then the xor butterfly for s = W/2, ..., 1.
 *       out[16b + 0..7]   = the record of ocean_body_buoyancy for the same hull, body, mode and K, bit for bit
 *       out[16b + 8..10]  = sum F          out[16b + 11..13] = sum T  (about the body origin c)
 *       out[16b + 14]     = fmaxf over the body's probes with f > 0 of m, from 0  (the largest relative speed on
 *                                                                                  the wet hull)
 *       out[16b + 15]     = sum wet        (the number of wet probes; exact: P <= 4096 < 2^24)
 * What a host does with a record: the drag force is k out[8..10] and the drag torque about c is k out[11..13],
 * k being the host's coefficient (density and wetted area per unit volume are folded into it, or into the
 * hull's v); out[14] against a threshold is a slam or spray trigger; out[15] = 0 means airborne.
 * Dry probes contribute g = 0 through the formulas as written, with no special case.  The library does not
 * inspect hull, body or motion values: non-finite inputs give unspecified numbers (never an access outside the
 * textures).  Before the first ocean_step VEL and DISP are zero and the entry is valid.
 *
 * The three forms are those of ocean_body_buoyancy: ocean_body_dynamics takes host buffers and blocks;
 * ocean_body_dynamics_device takes device pointers (hull, bodies and motion 4-B aligned, out 16-B aligned, else
 * OCEAN_E_INVALID_ARG), is async on the ctx stream and bounds count by OCEAN_BODY_MAX_SAMPLES alone;
 * ocean_body_dynamics_async consumes `hull`, `bodies` and `motion` before it returns, runs behind the steps
 * queued so far and lands count x 64 B in `out` through the readback slots, with the same
 * ocean_readback_status / _wait / _release / _copy_ms.  *req is NULL after every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for everything ocean_body_buoyancy refuses
 * (the same OCEAN_BODY_MAX_* limits), a null `motion` or a `law` that is neither OCEAN_DRAG_*; then
 * OCEAN_E_UNSUPPORTED on a context without OCEAN_F_VELOCITY, OCEAN_E_STATE before ocean_init_spectrum and
 * OCEAN_E_UNSUPPORTED on a column-parity context (as ocean_query_velocity).  count = 0 is a no-op in the
 * blocking and device forms and OCEAN_E_INVALID_ARG in the async form.  The launch counts as kind 2 of
 * ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_DRAG_LINEAR 0
#define OCEAN_DRAG_QUADRATIC 1
int ocean_body_dynamics(ocean_ctx *ctx, int tile, int mode, int iterations, int law, const float *hull, int probes,
                        const float *bodies, const float *motion, int count, float *out);
int ocean_body_dynamics_device(ocean_ctx *ctx, int tile, int mode, int iterations, int law, const float *hull,
                               int probes, const float *bodies, const float *motion, int count, float *out);
int ocean_body_dynamics_async(ocean_ctx *ctx, int tile, int mode, int iterations, int law, const float *hull,
                              int probes, const float *bodies, const float *motion, int count, float *out,
                              ocean_readback **req);

/* Surface bounds: how far the water of a tile can be from rest, per cascade.  A renderer needs them for
 * the bounding box of its displaced mesh (frustum culling, tessellation range; the reference leaves its
 * mesh bounds to Unity's defaults), and ocean_raycast below skips the air above them.
 *
 * `bytes` must equal C * 32.  Record c of `out` is float[8] = (min x, min y, min z, min w, max x, max y,
 * max z, max w) over the N * N texels of DISP slice tile * C + c, channel by channel (x = Dx, y = Dy, z = Dz,
 * w as the frame wrote it).  Min and max do not depend on the order of a reduction, so the numbers are
 * exact: those of a host that reads the slice back and takes the min and max itself (-0 and +0 compare
 * equal, and either may be returned).  NaN texels give unspecified numbers.  On a column-band context the
 * columns the context does not write (zero after ocean_create) take part like any other.
 * What a host forms from the records: sum_c min_c <= D(p) <= sum_c max_c, channel by channel and up to
 * rounding (a few ulp of sum_c max(|min_c|, |max_c|)), for the cascade-summed displacement D(p) that
 * ocean_sample_world returns at any point p, a bilinear tap lying between the texels it blends.  The
 * displaced mesh of a patch [x0, x1] x [z0, z1] therefore lies inside [x0 + sum min x, x1 + sum max x] x
 * [sum min y, sum max y] x [z0 + sum min z, z1 + sum max z].
 *
 * Cache.  The context keeps the records of a tile until an entry of this library writes DISP: ocean_step,
 * ocean_fill, ocean_write of OCEAN_TEX_DISP, ocean_set_column_band and ocean_set_column_parity drop them,
 * and the next use runs the two reduction kernels again (kind 2 of ocean_kernel_stats / ocean_kernel_name).
 * Once ocean_get_device_ptr(OCEAN_TEX_DISP) has handed the pointer out, the context caches nothing any more
 * and recomputes at every use, for the life of the context: a foreign writer cannot be seen.
 *
 * ocean_surface_bounds: `out` is a host buffer; blocks.  ocean_surface_bounds_device: `out` is a device
 * pointer, 16-B aligned (else OCEAN_E_INVALID_ARG); async on the ctx stream, ordered after the queued steps.
 * Both: OCEAN_E_INVALID_ARG, checked before any device call, for a null ctx or `out`, a tile out of range
 * or a wrong `bytes`; then OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a
 * column-parity context (as the queries). */
int ocean_surface_bounds(ocean_ctx *ctx, int tile, float *out, size_t bytes);
int ocean_surface_bounds_device(ocean_ctx *ctx, int tile, float *out, size_t bytes);

/* Ray casts: where a ray meets the water.  Every entry above starts from a known world (x, z); projectile
 * and spray impacts, mouse picking, camera and line-of-sight checks and range sensors start from a ray (the
 * water's analogue of Unity's Physics.Raycast; the reference has none).  Ray i of `rays` is float[8] =
 * (ox, oy, oz, dx, dy, dz, t0, t1): an origin, a direction and the parameter interval to search; out[i] is
 * float[8].  The library does not inspect the values: a non-unit direction scales t, and t1 < t0 marches
 * backwards.
 *
 * All arithmetic is fp32, one rounding per operation in the order written (no fused multiply-add).  With
 * K = `iterations` in [0, 16], S = `steps` in [1, OCEAN_RAY_MAX_STEPS], B = `refine` in [0, 32] and rec(x, z)
 * the 8-float record of OCEAN_QUERY_SURFACE for the point (x, z) of tile `tile` with K iterations, bit for bit:
 *
 *       pos(t) = (ox + t * dx,  oy + t * dy,  oz + t * dz)
 *       f(t)   = pos(t).y - rec(pos(t).x, pos(t).z)[0]            (height of the ray point over the water)
 *       dt     = (t1 - t0) / (float)S
 *       t_j    = t0 + (float)j * dt,   j = 0 .. S
 *
 *       if !(f(t_0) > 0):                     status = OCEAN_RAY_SUBMERGED, t* = t_0
 *       else for the first j in 1 .. S with !(f(t_j) > 0):
 *              a = t_(j-1), b = t_j;  B times:  m = 0.5f * (a + b);  if f(m) > 0: a = m  else: b = m
 *                                             status = OCEAN_RAY_HIT, t* = b
 *       else:                                 status = OCEAN_RAY_MISS, t* = t_S
 *
 *       R = rec(pos(t*).x, pos(t*).z)
 *       out[8i + 0..3] = t*,  pos(t*).y - R[0],  R[3],  (float)status
 *       out[8i + 4..7] = R[4..7]                                  (normal and foam at the point met)
 *
 * After a hit f(t*) <= 0 < f(a) and b - a = dt / 2^B up to rounding; the host forms the point met as
 * o + t* d.  out[8i + 1] is the ray point's height over the water there (<= 0 after a hit, the clearance at
 * t_S after a miss) and out[8i + 2] the fixed point's residual, as in the queries.
 * Limits of the method.  The march sees the surface only at its S + 1 nodes: a crest thinner than dt along
 * the ray can be stepped over, and S is the caller's resolution.  K has the meaning and the convergence
 * caveats of ocean_query_surface.  Non-finite inputs give unspecified numbers, never an access outside the
 * textures.
 * Air skip.  A node higher than every wave has f > 0 without a sample, and only the sign of f is used at a
 * node.  The kernel takes the height no wave reaches from ocean_surface_bounds' records of the tile (the sum
 * of the cascades' max y plus a derived rounding margin) and samples only the nodes at or below it; every
 * result bit is as defined above, only the time differs.  A ray cast on a context whose bounds are stale
 * (see their cache rule) first enqueues the two bounds kernels on the ctx stream.  OCEAN_RAY_BOUNDS=0 in the
 * environment (read by ocean_create) turns the skip and those launches off, here, in ocean_camera* and in
 * ocean_spray_step*, which skip the same way.
 *
 * The three forms, their ordering and `*req` are those of ocean_query_surface, ocean_query_surface_device and
 * ocean_query_surface_async: ocean_raycast takes host buffers and blocks; ocean_raycast_device takes device
 * pointers (rays 4-B aligned, out 16-B aligned, else OCEAN_E_INVALID_ARG) and is async on the ctx stream,
 * ordered after the queued steps; ocean_raycast_async consumes the host buffer `rays` before it returns, runs
 * on the ctx stream after the steps queued so far and before later ones, and lands count x 32 B in `dst` on
 * the copy stream through the same readback slots, with the same ocean_readback_status / _wait / _release /
 * _copy_ms.  *req is NULL after every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null ctx, rays, out or req, count < 0,
 * count > OCEAN_RAY_MAX_RAYS (host and async forms, which stage the rays), steps outside
 * [1, OCEAN_RAY_MAX_STEPS], count * steps > OCEAN_RAY_MAX_SAMPLES (in 64 bits, all forms), iterations outside
 * [0, 16], refine outside [0, 32] or a tile out of range; then OCEAN_E_STATE before ocean_init_spectrum and
 * OCEAN_E_UNSUPPORTED on a column-parity context (as the queries).  count = 0 is a no-op in the blocking and
 * device forms and OCEAN_E_INVALID_ARG in the async form (there is no request to hand back). */
#define OCEAN_RAY_MISS 0
#define OCEAN_RAY_HIT 1
#define OCEAN_RAY_SUBMERGED 2
#define OCEAN_RAY_MAX_RAYS 16384
#define OCEAN_RAY_MAX_STEPS 1024
#define OCEAN_RAY_MAX_SAMPLES (1 << 24)
int ocean_raycast(ocean_ctx *ctx, int tile, int iterations, int steps, int refine, const float *rays, int count,
                  float *out);
int ocean_raycast_device(ocean_ctx *ctx, int tile, int iterations, int steps, int refine, const float *rays,
                         int count, float *out);
int ocean_raycast_async(ocean_ctx *ctx, int tile, int iterations, int steps, int refine, const float *rays,
                        int count, float *dst, ocean_readback **req);

/* Whitecap emitters: where the sea is breaking.  Every entry above answers "what is the water doing here?" for a
 * place the host already knows; a spray, foam-particle or audio system asks where to spawn, every frame.  The
 * reference has the foam only as a shading term (Water.shader:343 sums 1 - saturate(TURB.x) over the cascades); a
 * host that wants emitters would read the TURB slices back, or a dense OCEAN_GRID_VERTICES grid at 32 B per node,
 * to threshold a few hundred nodes out of them.  Here the threshold and the compaction run on the device and
 * (capacity + 1) x 32 B come back.
 *
 * The grid is ocean_surface_grid's six numbers with the same node arithmetic: node (i, j), i < nx, j < ny, lies at
 *       q.x = x0 + (float)i * dx,   q.z = z0 + (float)j * dz     (one fp32 multiply and one fp32 add each)
 * and has the index k = j * nx + i.  Zero and negative spacings are valid.  With S(q) what ocean_sample_world
 * returns for the point (q.x, q.z, lod) of tile `tile` (TURB at `lod` exactly as there: trilinear on OCEAN_F_MIPS
 * contexts, level 0 otherwise):
 *       foam(k) = S(q)[3]
 *       node k is selected iff foam(k) >= threshold      (an fp32 compare: a NaN foam is never selected)
 *       T = the number of selected nodes,   rank(k) = the number of selected nodes k' < k
 *
 * `out` holds capacity + 1 records of 32 B; `bytes` must equal (capacity + 1) * 32.  Record 0 is a header of eight
 * uint32: T, W = min(T, capacity), nx * ny, capacity, 0, 0, 0, 0.  Every selected node with rank(k) < capacity
 * writes record 1 + rank(k), eight floats:
 *       [0..3] = q.x + S(q)[0], S(q)[1], q.z + S(q)[2], foam(k)    (bit for bit the first four floats of the
 *                                                                   OCEAN_GRID_VERTICES record of that node at that lod)
 *       [4..6] = Vs(q).xyz, exactly out[0..2] of ocean_query_velocity for q with iterations = 0, on an
 *                OCEAN_F_VELOCITY context; +0, +0, +0 on any other
 *       [7]    = (float)k                                          (exact: k < 2^22)
 * The records come out in ascending k.  On overflow (T > capacity) the first `capacity` selected nodes in k order
 * are kept and T still counts every selected node, so a host sees how much it missed.  Records W + 1 .. capacity
 * are not written; their contents are unspecified.  The result does not depend on the launch grid or on
 * scheduling: three launches (count, scan, emit; kind 2 of ocean_kernel_stats / ocean_kernel_name) with no atomics
 * and no workgroup that waits for another.  Their scratch (at most 576 KiB) belongs to the context: allocated by
 * the first call of any form, reused by every later one, freed by ocean_destroy.
 *
 * ocean_whitecaps: `out` is a host buffer; blocks, as ocean_surface_grid.
 * ocean_whitecaps_device: `out` is a device pointer, 16-B aligned (else OCEAN_E_INVALID_ARG); async on the ctx
 * stream, ordered after the queued steps: a particle system on the device reads the list with no host copy.
 * ocean_whitecaps_async: `out` is a host destination (pinned, ocean_host_alloc, for a truly asynchronous copy).  The
 * list is built in a readback slot on the ctx stream, after the steps queued so far and before later ones, and all
 * (capacity + 1) * 32 bytes (at most 2 MiB: every list fits a slot) are copied on the copy stream like an
 * ocean_read_async slice, with the same ocean_readback_status / _wait / _release / _copy_ms.  *req is NULL after
 * every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null ctx, `out` or `req`, a tile out of
 * range, a lod that is not finite or negative, a non-finite threshold, x0, z0, dx or dz, nx < 1 or ny < 1,
 * nx * ny > OCEAN_GRID_MAX_NODES (in 64 bits), capacity outside [1, OCEAN_WHITECAP_MAX_RECORDS], a wrong `bytes` or
 * a misaligned device `out`; then, in this order, OCEAN_E_UNSUPPORTED on a DISPLACEMENT_ONLY context (it has no
 * TURB), OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context (as the
 * queries). */
#define OCEAN_WHITECAP_MAX_RECORDS 65535
int ocean_whitecaps(ocean_ctx *ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                    int nx, int ny, int capacity, float *out, size_t bytes);
int ocean_whitecaps_device(ocean_ctx *ctx, int tile, float lod, float threshold, float x0, float z0, float dx,
                           float dz, int nx, int ny, int capacity, float *out, size_t bytes);
int ocean_whitecaps_async(ocean_ctx *ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz,
                          int nx, int ny, int capacity, float *out, size_t bytes, ocean_readback **req);

/* Camera views: an image of the sea.  The fragment stage of Water.shader (:336-374) is what the reference's
 * textures exist for, and a host on a device without a display pipeline has no picture of them: with ocean_raycast
 * it would build width x height rays on the CPU, upload and read back 32 B per pixel, sample DERIV and TURB again
 * at a distance-dependent lod and shade on the CPU.  Maritime camera and lidar sensors, regression pictures,
 * previews and training data need the image itself.  Here the rays follow from a camera of fourteen numbers, as a
 * grid follows from six; the march, the sample and the shading are one kernel, and 4, 16 or 32 B per pixel come
 * back.
 *
 * `camera` is float[OCEAN_CAMERA_FLOATS] = (o.x, o.y, o.z, d00.x, d00.y, d00.z, du.x, du.y, du.z, dv.x, dv.y, dv.z,
 * t0, t1): the eye, the unnormalised direction through pixel (0, 0), its change per pixel along a row and along a
 * column, and the parameter interval every ray searches.  Pixel (i, j), i < width and j < height, is element
 * k = j * width + i of `out`.  All arithmetic is fp32, one rounding per operation in the order written (no fused
 * multiply-add); sqrtf and / are correctly rounded.
 *       raw = (d00 + (float)i * du) + (float)j * dv                     (componentwise)
 *       len = sqrtf((raw.x * raw.x + raw.y * raw.y) + raw.z * raw.z)
 *       d   = (raw.x / len, raw.y / len, raw.z / len)
 * The pixel's ray is (o, d, t0, t1), and R_k is the 8-float record of ocean_raycast for that ray with the same
 * `tile`, `iterations` (K), `steps` (S) and `refine` (B), bit for bit.  The air skip, the bounds launches on a
 * context whose bounds are stale and OCEAN_RAY_BOUNDS=0 are exactly ocean_raycast's.  The library does not inspect
 * what the camera spans: len = 0 gives unspecified numbers (never an access outside the textures).
 *
 *   OCEAN_CAMERA_HITS:  out[8k + 0..7] = R_k: the G-buffer, 32 B per pixel.
 *   OCEAN_CAMERA_RANGE: out[k] = R_k[0] after a hit or a submerged start, +INFINITY after a miss: a range or lidar
 *                       image, 4 B per pixel.
 *   OCEAN_CAMERA_COLOR: out[4k + 0..3] = (r, g, b, (float)status): the shaded picture, 16 B per pixel.
 * `bytes` must equal width * height * 32, 4 or 16.  `material` is read in colour mode only and may be NULL in the
 * other two.
 *
 * `material` is float[OCEAN_CAMERA_MATERIAL_FLOATS]; the names in brackets are Water.shader's properties:
 *       [0..2]   C      the water colour (_Color)
 *       [3]      R0     the reflectance at normal incidence (the shader's R0: ((1 - 1.333) / (1 + 1.333))^2)
 *       [4]      FE     the Fresnel exponent 5 exp(-2.69 roughness)                 (:353)
 *       [5]      FD     the Fresnel divisor 1 + 22.7 roughness^1.5                  (:353)
 *       [6]      rho    the roughness (_Roughness)
 *       [7]      lod_slope: levels of detail per unit of distance along the ray (the role of _MaxLODLevel /
 *                _MaxTesselationDistance, :319-320)
 *       [8], [9] EX, EY (_EX, _EY)
 *       [10]     ke     the environment reflection strength (_EnvironmentReflectionStrength)
 *       [11]     ks     the sun reflection strength (_SunReflectionStrength)
 *       [12..14] SS     the subsurface colour times the subsurface intensity (_SubsurfaceScatteringColor.rgb *
 *                       _SubsurfaceScatteringIntensity): the bindings take the two apart and multiply once
 *       [15]     FT     the foam threshold (_FoamThreshold)
 *       [16..18] FC     the foam colour (_FoamColor)
 *       [19]     FB     the foam blending (_FoamBlending)
 *       [20..22] L      the direction towards the light, unit (the caller keeps it so)
 *       [23..25] LC     the light's colour (_MainLightColor)
 *       [26..28] HZ     the sky's colour at and below the horizon
 *       [29..31] ZN     the sky's colour at the zenith
 * FE and FD are the material's only transcendentals: whoever builds the material computes them once, and the
 * kernel evaluates none per material.
 *
 * The colour is the fragment stage restated in fp32 in the order written, with these definitions of the library's
 * own where the shader reads what a headless host does not have:
 *   - view and lod: V = -d, and the pixel's lod = R_k[0] * lod_slope (the distance along the ray in place of
 *     :319-320's distance to the camera);
 *   - the surface sample is taken at the point the fixed point ended on: with q = o + R_k[0] * d and p_K the
 *     fixed point of OCEAN_QUERY_SURFACE for (q.x, q.z) after K steps, S = ocean_sample_world's result for
 *     (p_K.x, p_K.z, lod): n = S[8..10], foam = S[3], eta = S[1].  DERIV and TURB use `lod` exactly as
 *     ocean_sample_world does (trilinear on OCEAN_F_MIPS contexts, level 0 otherwise, a lod <= 0 is level 0);
 *   - no shadow map: the shadow factor is 1, so the sun's lobes are not attenuated and the shadow lerp of :370
 *     (whose weight is then 0) is left out, _ShadowsColor and _ShadowsIntensity with it;
 *   - no opaque or depth texture: UnderwaterView is its fog limit, the water colour;
 *   - no cubemap: sky(r) = HZ + saturate(r.y) * (ZN - HZ), per channel (with OCEAN_CAMERA_SKY_LUT: the atmosphere's
 *     sky-view table, "The atmosphere" below).
 * With sat(x) = fminf(fmaxf(x, 0), 1), dot(a, b) = (a.x * b.x + a.y * b.y) + a.z * b.z, pi = (float)3.14159265358979
 * and tiny = 1.175494351e-38f, a HIT pixel is
 *       hr  = V + L;   h = hr / sqrtf(dot(hr, hr))                                  (the halfway vector, three divisions)
 *       ndv = dot(n, V);  ndl = dot(n, L);  hdv = dot(h, V);  hdn = dot(h, n)
 *       F   = R0 + ((1 - R0) * powf(1 - sat(ndv), FE)) / FD                         (:353)
 *       x   = 1 - sat(hdv);   FH = R0 + (1 - R0) * (((x * x) * (x * x)) * x)        (:354)
 *       s   = fmaxf(0, dot(L, d));   g = fmaxf(0, eta) * ((s * s) * (s * s))        (subsurface: dot(L, -V), :176)
 *       refraction_c = C_c + (g * SS_c) * LC_c
 *       ry  = (2 * ndv) * n.y - V.y                                                 (-reflect(V, n), its y)
 *       env_c = (sky(ry)_c * pi) * ke                                               (:187)
 *     if L.y > 0 (else cook_c = 0 and ash_c = 0, :215 and :225):
 *       den = fmaxf(1 - h.z * h.z, tiny);  c2 = fmaxf((h.x * h.x) / den, 0);  s2 = fmaxf((h.y * h.y) / den, 0)
 *       nu  = (EX * 10) * (1 - rho);   nv = (EY * 10) * (1 - rho)
 *       D   = sqrtf((nu + 1) * (nv + 1)) * powf(fmaxf(hdn, 0), nu * c2 + nv * s2)
 *       A   = fmaxf((D * FH) / fmaxf(((8 * pi) * hdv) * fmaxf(ndv, ndl), tiny), 0);   ash_c = LC_c * A     (:226-230)
 *       a2  = (rho * rho) * (rho * rho);   q = (sat(hdn) * sat(hdn)) * (a2 - 1) + 1
 *       N   = fmaxf(a2 / fmaxf(pi * (q * q), tiny), 0);   k = rho / 2                                      (:192-196)
 *       G   = fmaxf((sat(ndv) / fmaxf(sat(ndv) * (1 - k) + k, tiny)) * (sat(ndl) / fmaxf(sat(ndl) * (1 - k) + k, tiny)), 0)
 *       cook_c = ((LC_c * N) * G) / fmaxf((8 * sat(ndv)) * sat(ndl), tiny)                                 (:219)
 *     then
 *       reflections_c = env_c + (cook_c + ash_c * sat(ndv)) * ks                    (:368)
 *       e_c = refraction_c + F * (reflections_c - refraction_c)                     (:370)
 *       if foam >= FT:  e_c = e_c + FB * (FC_c - e_c)                               (:371)
 *       (r, g, b) = e
 * The shader's quirks are kept: the Ashikhmin-Shirley angles are taken in the world's x and y, FH feeds only that
 * lobe, and the lobes are clamped, not the sum.  Integer powers are the multiplications written; the two powf are
 * the only operations whose last bits depend on the device's math library.  A MISS pixel is sky(d.y) and a
 * SUBMERGED pixel is C, both with their status in the fourth channel.  A DISPLACEMENT_ONLY context shades with
 * n = (0, 1, 0) and never foams, as the queries report it.
 *
 * ocean_camera: `out` is a host buffer; blocks, as ocean_surface_grid.
 * ocean_camera_device: `out` is a device pointer, 16-B aligned in every mode (else OCEAN_E_INVALID_ARG); async on
 * the ctx stream, ordered after the queued steps.
 * ocean_camera_async: `out` is a host destination (pinned, ocean_host_alloc, for a truly asynchronous copy).  The
 * image is computed into a readback slot on the ctx stream, after the steps queued so far and before later ones,
 * and copied on the copy stream like an ocean_read_async slice, with the same ocean_readback_status / _wait /
 * _release / _copy_ms.  The result must fit a slot: bytes <= max(N * N * 16, OCEAN_QUERY_MAX_POINTS * 40), else
 * OCEAN_E_INVALID_ARG.  *req is NULL after every failure.
 * In all three `camera` and `material` are host arrays, consumed before the call returns and passed to the kernel
 * by value: nothing is staged.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null ctx, `camera`, `out` or `req`, a null
 * `material` in colour mode, a tile out of range, an unknown mode, iterations outside [0, 16], steps outside
 * [1, OCEAN_RAY_MAX_STEPS], refine outside [0, 32], a non-finite camera value or a non-finite value of a `material` that is passed (in any mode),
 * width < 1 or height < 1, width * height > OCEAN_CAMERA_MAX_PIXELS, width * height * steps >
 * OCEAN_CAMERA_MAX_SAMPLES (both in 64 bits), a wrong `bytes`, a misaligned device `out` or an async result larger
 * than a slot; then OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context (as
 * the queries).  The launch counts as kind 2 of ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_CAMERA_HITS 0
#define OCEAN_CAMERA_RANGE 1
#define OCEAN_CAMERA_COLOR 2
#define OCEAN_CAMERA_FLOATS 14
#define OCEAN_CAMERA_MATERIAL_FLOATS 32
#define OCEAN_CAMERA_MAX_PIXELS (1 << 22)
#define OCEAN_CAMERA_MAX_SAMPLES (1 << 28)
#define OCEAN_CAMERA_SKY_LUT 16 /* valid only as OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT: see "The atmosphere" below */
int ocean_camera(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine, const float *camera,
                 const float *material, int width, int height, float *out, size_t bytes);
int ocean_camera_device(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine, const float *camera,
                        const float *material, int width, int height, float *out, size_t bytes);
int ocean_camera_async(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine, const float *camera,
                       const float *material, int width, int height, float *out, size_t bytes, ocean_readback **req);

/* Body steps: ocean_body_dynamics with the integrator behind it and a loop of S substeps around both, so that M
 * rigid bodies advance S substeps in one launch and their state never leaves the device.  The reference's
 * BuoyantObject.FixedUpdate runs several fixed updates per rendered frame against one frame of water; a host that
 * does the same with the entries above pays, per substep, one latency-bound launch, a readback of the wrenches, the
 * integration of M bodies on the CPU and an upload of their poses and motions.  Here a renderer reads the poses from
 * a device pointer, and a host reads 128 B per body once per frame.  Needs a context created with OCEAN_F_VELOCITY.
 *
 *   hull:   float[P][5], exactly as ocean_body_buoyancy takes it.
 *   state:  record b is float[32]: [0..9] = (c, q, s) as a `bodies` record of ocean_body_buoyancy, [10..15] = (v, o)
 *           as a `motion` record of ocean_body_dynamics, [16..31] ignored.
 *   props:  body b is float[4] = (im, jx, jy, jz): the inverse mass and the inverse principal moments of inertia in
 *           the body frame.  A zero makes the body immovable by forces in that degree of freedom (g, an acceleration,
 *           acts whatever im is: a body at rest for good has im = 0 in a call whose step has g = 0, or is left out).
 *   step:   float[OCEAN_BODY_STEP_FLOATS] = (h, g, B, kd, kt, la, aa, 0), a host array in every form, read before the
 *           call returns (like ocean_camera's `camera`): the substep in seconds, gravity's magnitude, the buoyant
 *           force per unit of submerged volume (rho g), the coefficients of the drag force and the drag torque (the
 *           host's k of the dynamics record), and the reference's `drag` and `angularDrag`, which damp against still
 *           water while any probe is wet.  step[7] is reserved: pass 0.
 *   out:    record b is float[32]: [0..15] = the state after `substeps` substeps, in the layout of `state`;
 *           [16..31] = the ocean_body_dynamics record of the last substep, taken at the state that substep started
 *           from.  `out` of one call is `state` of the next.
 *
 * All arithmetic is fp32, each line one rounding per operation in the order written (no fused multiply-add); sqrtf
 * and / are correctly rounded.  With (u x a) = (u.y * a.z - u.z * a.y,  u.z * a.x - u.x * a.z,  u.x * a.y - u.y * a.x)
 * and rot(u, w, a) the rotation ocean_body_buoyancy applies to a probe:
 *       t = (2 * (u x a).x, 2 * (u x a).y, 2 * (u x a).z),    rot(u, w, a) = (a + w * t) + (u x t), componentwise
 * one substep takes c, q = (u, qw) with u = (qx, qy, qz), s, v, o to c', q', s', v', o':
 *       rec  = the 16-float record of ocean_body_dynamics for (hull, (c, q, s), (v, o), mode, iterations, law), bit
 *              for bit (the same lanes, trip count and butterfly)
 *       acc  = (im * (kd * rec[8]),   im * (B * rec[0] + kd * rec[9]) - g,   im * (kd * rec[10]))
 *       tau  = (kt * rec[11] - B * rec[3],   kt * rec[12],   kt * rec[13] + B * rec[1])
 *       tb   = rot((-u.x, -u.y, -u.z), qw, tau)                       (the torque in the body frame)
 *       alp  = rot(u, qw, (jx * tb.x, jy * tb.y, jz * tb.z))          (no gyroscopic term, by definition)
 *       v'   = (v.x + h * acc.x, v.y + h * acc.y, v.z + h * acc.z)
 *       o'   = (o.x + h * alp.x, o.y + h * alp.y, o.z + h * alp.z)
 *       if rec[15] > 0:   v'.i = v'.i - (v.i * la) * h,   o'.i = o'.i - (o.i * aa) * h   for i = x, y, z
 *                                                     (the v and o the substep started from: a VelocityChange)
 *       c'   = (c.x + h * v'.x, c.y + h * v'.y, c.z + h * v'.z)
 *       hh   = 0.5f * h
 *       n.i  = u.i + hh * (qw * o'.i + (o' x u).i)   for i = x, y, z
 *       nw   = qw - hh * ((o'.x * u.x + o'.y * u.y) + o'.z * u.z)
 *       len  = sqrtf(((n.x * n.x + n.y * n.y) + n.z * n.z) + nw * nw)
 *       q'   = (n.x / len, n.y / len, n.z / len, nw / len),   s' = s
 * (semi-implicit Euler: the new velocity moves the body; dq/dt = (o, 0) q / 2 with o in the world frame, then
 * renormalised).  Substep k + 1 starts from the result of substep k.  The water (DISP, DERIV, VEL) is the frame's and
 * the same for every substep of a call, as it is for the reference's fixed updates between two Updates.  The
 * reference's FixedUpdate is the one-probe hull (0, 0.5, 0, 1, 1) in reference mode with im = 1, kd = kt = 0,
 * B = g * density, la = drag, aa = angularDrag.  The library does not inspect hull, state or props values:
 * non-finite inputs give unspecified numbers (never an access outside the textures).  Before the first ocean_step
 * VEL and DISP are zero and the entry is valid.
 *
 * The three forms are those of ocean_body_dynamics: ocean_body_step takes host buffers and blocks;
 * ocean_body_step_device takes device pointers for hull, props, state and out (inputs 4-B aligned, out 16-B aligned,
 * else OCEAN_E_INVALID_ARG), is async on the ctx stream and bounds count by the sample limits alone; it allows
 * out == state (in place): only the lanes of body b read or write record b, and they read before they write.  Any
 * other overlap of out with an input is undefined.  ocean_body_step_async consumes `hull`, `props` and `state`
 * before it returns, runs behind the steps queued so far and lands count x 128 B in `out` through the readback
 * slots, with the same ocean_readback_status / _wait / _release / _copy_ms.  *req is NULL after every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for everything ocean_body_dynamics refuses (the
 * same OCEAN_BODY_MAX_* limits, `state` in the place of `bodies`), a null `step`, `props` or `state`, a `step` value
 * that is not finite, substeps outside [1, OCEAN_BODY_MAX_SUBSTEPS] or count * probes * substeps >
 * OCEAN_BODY_STEP_MAX_SAMPLES (in 64 bits); then OCEAN_E_UNSUPPORTED on a context without OCEAN_F_VELOCITY,
 * OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context.  count = 0 is a
 * no-op in the blocking and device forms and OCEAN_E_INVALID_ARG in the async form.  The launch counts as kind 2 of
 * ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_BODY_STEP_FLOATS 8
#define OCEAN_BODY_MAX_SUBSTEPS 64
#define OCEAN_BODY_STEP_MAX_SAMPLES (1 << 24)
int ocean_body_step(ocean_ctx *ctx, int tile, int mode, int iterations, int law, int substeps, const float *step,
                    const float *hull, int probes, const float *props, const float *state, int count, float *out);
int ocean_body_step_device(ocean_ctx *ctx, int tile, int mode, int iterations, int law, int substeps, const float *step,
                           const float *hull, int probes, const float *props, const float *state, int count,
                           float *out);
int ocean_body_step_async(ocean_ctx *ctx, int tile, int mode, int iterations, int law, int substeps, const float *step,
                          const float *hull, int probes, const float *props, const float *state, int count, float *out,
                          ocean_readback **req);

/* Mesh hulls: the hydrostatic pressure integrated over the wetted part of a triangle mesh, for M rigid bodies that
 * share the mesh, reduced on the device to 64 B per body whatever the mesh's size.  A probe of ocean_body_buoyancy is a
 * vertical column: it has no side, so it cannot place the waterline on a sloped plate; its horizontal force is zero, so
 * a hull never feels the slope of the wave it sits on (the Froude-Krylov surge and sway); it has neither wetted nor
 * waterplane area; and its accuracy is that of the host's voxelisation.  Here the water is sampled over the mesh's
 * vertices, every triangle is clipped at the waterline and the pressure, taken as linear over a clipped piece, is
 * integrated exactly.  With the entries above a host would query M x V points, read M x V x 32 B back and clip itself.
 *
 *   vertices:  vertex i is float[3] = (rx, ry, rz) in the body frame.  V = nverts in [1, OCEAN_HULL_MAX_VERTICES].
 *   triangles: triangle k is int[3] = (i0, i1, i2), indices into `vertices`, counter-clockwise seen from outside (the
 *              normal (P1 - P0) x (P2 - P0) points out of the hull).  T = ntris in [1, OCEAN_HULL_MAX_TRIANGLES].
 *              Declared `const void *` so that every binding marshals it as a plain address; it is an int array.
 *   bodies:    float[M][10], exactly as ocean_body_buoyancy takes it.
 *   out:       record b is float[OCEAN_HULL_RECORD_FLOATS] = float[16].
 * The surface lookup is always OCEAN_QUERY_SURFACE with K = `iterations` in [0, 16]; there is no mode argument, because
 * a texel pick has no waterline.
 *
 * All arithmetic is fp32, each line one rounding per operation in the order written (no fused multiply-add); sqrtf and /
 * are correctly rounded.  (a x b) = (a.y * b.z - a.z * b.y,  a.z * b.x - a.x * b.z,  a.x * b.y - a.y * b.x), and a
 * vector line is meant componentwise.
 * Per vertex i of body b: a, t, d_i and w_i = c + d_i exactly as ocean_body_buoyancy defines them for a probe's
 * (rx, ry, rz); rec = the 8-float record of ocean_query_surface for the point (w.x, w.z) with K iterations, bit for bit;
 *       z_i = rec[0] - w_i.y          (the depth of the vertex, positive when submerged)
 *       r_i = rec[3]
 * Per triangle (i0, i1, i2): P_k = d_ik (positions relative to the body origin), z_k the depths.  A vertex is wet iff
 * z > 0 (so z = +0 and z = -0 are dry), and m is the number of wet vertices.
 *       m = 0: nothing.
 *       m = 3: one piece (P0, P1, P2; z0, z1, z2).
 *       m = 1: (A, B, C) = (P0, P1, P2), (P1, P2, P0) or (P2, P0, P1), whichever has the wet vertex first;
 *              AB = A + (zA / (zA - zB)) * (B - A),   AC = A + (zA / (zA - zC)) * (C - A);
 *              one piece (A, AB, AC; zA, 0, 0).
 *       m = 2: (A, B, C) = (P0, P1, P2), (P1, P2, P0) or (P2, P0, P1), whichever has the dry vertex last;
 *              BC = B + (zB / (zB - zC)) * (C - B),   CA = A + (zA / (zA - zC)) * (C - A);
 *              two pieces, (A, B, BC; zA, zB, 0) and then (A, BC, CA; zA, 0, 0).
 *       (X + (zX / (zX - zY)) * (Y - X) is, per component, X.x + t * (Y.x - X.x) with t = zX / (zX - zY) formed once;
 *        zX > 0 >= zY whenever it is formed, so the divisor is positive.)
 * Per piece (Q0, Q1, Q2; y0, y1, y2):
 *       Av = 0.5f * ((Q1 - Q0) x (Q2 - Q0))                          (the area vector, outward)
 *       S  = (y0 + y1) + y2,   p = S / 3
 *       F  = -(p * Av)                                                (the integral of -depth n dA)
 *       Mo = ((Q0 * (y0 + S) + Q1 * (y1 + S)) + Q2 * (y2 + S)) / 12   (the integral of depth r dA, over the area)
 *       Tq = -(Mo x Av)                                               (the integral of r x (-depth n) dA)
 *       ar = sqrtf((Av.x * Av.x + Av.y * Av.y) + Av.z * Av.z)
 *       G  = ar * (((Q0 + Q1) + Q2) / 3)
 * The sums are defined exactly.  There are 256 lanes.  Lane l accumulates each term from +0, t_l = t_l + term, over its
 * triangles k = l, l + 256, ... in ascending order, within a triangle piece 1 and then piece 2; the vertex maxima and
 * the vertex count run over i = l, l + 256, ... alike.  Then for s = 128, 64, ..., 1: t_l = t_l + t_(l xor s) for every
 * l (fmaxf for the maxima); the result is t_0.  (In numpy: fold the upper half of t onto the lower half until one is
 * left, as for ocean_body_buoyancy but always over 256 lanes.)
 *       out[16b + 0..2]   = sum F           (times rho g: the hydrostatic force)
 *       out[16b + 3]      = sum ar          (the wetted area)
 *       out[16b + 4..6]   = sum Tq          (times rho g: the torque about the body origin c)
 *       out[16b + 7]      = fmaxf over the vertices of r_i, from 0
 *       out[16b + 8..10]  = sum G           (the wetted area's first moment about c)
 *       out[16b + 11]     = the number of triangles with m > 0
 *       out[16b + 12]     = fmaxf over the vertices of z_i, from 0        (the draught)
 *       out[16b + 13]     = the number of wet vertices
 *       out[16b + 14]     = sum Av.y        (its negative is the waterplane area of a closed hull)
 *       out[16b + 15]     = 0
 * The two counts are exact (at most 4096 < 2^24).  For a closed hull under flat water sum F = (0, V, 0) with V the
 * submerged volume (Archimedes), and sum Tq = (the centre of buoyancy - c) x sum F.  Under waves sum F.x and sum F.z are
 * the Froude-Krylov surge and sway.  Heave stiffness is rho g times the waterplane area, -out[14].
 * The library does not inspect vertex or body values: non-finite inputs give unspecified numbers (never an access
 * outside the textures or the vertex array).  A degenerate triangle adds zero to every sum.  Before the first
 * ocean_step the water is flat at 0 and the entry is valid; OCEAN_F_DISPLACEMENT_ONLY contexts are valid (only DISP is
 * read).
 *
 * The three forms are those of ocean_body_buoyancy.  ocean_body_hydrostatics takes host buffers and blocks.
 * ocean_body_hydrostatics_device takes device pointers (vertices, triangles and bodies 4-B aligned, out 16-B aligned,
 * else OCEAN_E_INVALID_ARG), is async on the ctx stream and bounds count by OCEAN_BODY_MAX_SAMPLES alone; it cannot see
 * the indices, so its kernel clamps each index into [0, nverts) and never reads outside the vertex array.
 * ocean_body_hydrostatics_async consumes its three arrays before it returns, runs behind the steps queued so far and
 * lands count x 64 B in `out` through the readback slots, with the same ocean_readback_status / _wait / _release /
 * _copy_ms.  *req is NULL after every failure.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, the entry's own arguments first and then the context
 * (as ocean_body_step): a null vertices, triangles, bodies, out or req, iterations outside [0, 16], nverts outside
 * [1, OCEAN_HULL_MAX_VERTICES], ntris outside [1, OCEAN_HULL_MAX_TRIANGLES], count < 0, count > OCEAN_BODY_MAX_BODIES
 * (host and async forms, which stage the bodies), count * nverts > OCEAN_BODY_MAX_SAMPLES (in 64 bits), a misaligned
 * device pointer, in the host and async forms an index outside [0, nverts), a null ctx, a tile out of range; then
 * OCEAN_E_STATE before ocean_init_spectrum and OCEAN_E_UNSUPPORTED on a column-parity context (as the queries).
 * count = 0 is a no-op in the blocking and device forms and OCEAN_E_INVALID_ARG in the async form.  The launch counts
 * as kind 2 of ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_HULL_MAX_VERTICES 2048
#define OCEAN_HULL_MAX_TRIANGLES 4096
#define OCEAN_HULL_RECORD_FLOATS 16
int ocean_body_hydrostatics(ocean_ctx *ctx, int tile, int iterations, const float *vertices, int nverts,
                            const void *triangles, int ntris, const float *bodies, int count, float *out);
int ocean_body_hydrostatics_device(ocean_ctx *ctx, int tile, int iterations, const float *vertices, int nverts,
                                   const void *triangles, int ntris, const float *bodies, int count, float *out);
int ocean_body_hydrostatics_async(ocean_ctx *ctx, int tile, int iterations, const float *vertices, int nverts,
                                  const void *triangles, int ntris, const float *bodies, int count, float *out,
                                  ocean_readback **req);

/* The atmosphere: the sky a sea picture reflects, and the colour of the light on it.  In the reference scene the
 * water's environment term (Water.shader:181-187) reads a reflection probe of the skybox, which is Atmosphere.shader
 * over the sky-view table of AtmosphereController.cs, and the light's colour comes from the transmittance table
 * (AtmosphereController.cs:129-154, :187-188).  Its three compute shaders are restated here; the context owns the three
 * tables, and OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT shades with the third in place of the two-colour sky.
 *
 * `params` is float[OCEAN_ATMOSPHERE_FLOATS], a host array read before the call returns and passed to the kernels by
 * value (like `camera`); the names are AtmosphereController's fields, the defaults its own:
 *       [0]      Rp     planetRadius 6360000                     [1]      Ra     atmosphereRadius 6420000
 *       [2..4]   RS     rayleighScatteringCoefficient (5.802e-6, 13.558e-6, 6.5e-5)
 *       [5..7]   RA     rayleighAbsorptionCoefficient (0, 0, 0)   [8]      HR     rayleighScaleHeight 8000
 *       [9..11]  MS     mieScatteringCoefficient (3.996e-6 x 3)
 *       [12..14] MA     mieAbsorptionCoefficient (4.4e-6 x 3)     [15]     HM     mieScaleHeight 1200
 *       [16]     g      0.85
 *       [17..19] OS     ozoneScatteringCoefficient (0, 0, 0)      [20..22] OA     ozoneAbsorptionCoefficient (0.65e-6, 1.881e-6, 0.085e-6)
 *       [23..25] GA     groundAlbedo (0, 0, 0)
 *       [26]     SZ     _SunSize of Atmosphere.shader, 0.04
 *       [27..31] reserved: pass 0
 *
 * A table is float4 per texel (the reference's ARGBFloat), row-major: texel (x, y) of a W x H table is element
 * y * W + x.  All arithmetic is fp32, one rounding per operation in the order written (no fused multiply-add); sqrtf
 * and / are correctly rounded; expf, sinf, cosf, acosf, atan2f, asinf and powf are the device library's.
 * PI = 3.14159265f (the compute shaders' own constant).  Shared by the three tables, per channel c:
 *       RE_c = RS_c + RA_c;   ME_c = MS_c + MA_c;   OE_c = OS_c + OA_c                   (the extinction coefficients)
 *       at the height h:  dr = expf((-h) / HR);  dm = expf((-h) / HM);  dz = fmaxf(0, 1 - (h - 25000) / 15000)
 *       ext_c(h) = (RE_c * dr + ME_c * dm) + OE_c * dz;     sca_c(h) = (RS_c * dr + MS_c * dm) + OS_c * dz
 *       texel (x, y) of a W x H table:  rad = (((float)x + 0.5f) / (float)W) * (Ra - Rp) + Rp,
 *                                        mu  = -1 + (((float)y + 0.5f) / (float)H) * 2
 *       clamp01(a) = fminf(fmaxf(a, 0), 1)
 * LUT reads (the reference's SampleLevel through a clamped bilinear sampler, restated as fp32 bilinear; hardware
 * filtering's fixed-point weights are not reproduced).  READ(L, u, v) of a W x H table L:
 *       X = fminf(fmaxf(clamp01(u) * (float)W - 0.5f, 0), (float)(W - 1));  x0 = (int)X;  x1 = min(x0 + 1, W - 1);  fx = X - (float)x0
 *       Y, y0, y1, fy alike from v and H                                     (texel centres at (i + 0.5) / W)
 *       lo = L[y0][x0] + fx * (L[y0][x1] - L[y0][x0]);   hi = L[y1][x0] + fx * (L[y1][x1] - L[y1][x0])
 *       READ = lo + fy * (hi - lo)                                           (x first, then y; per channel)
 *       LUTAT(L, sr, cosA) = READ(L, (sr - Rp) / (Ra - Rp), 0.5f + 0.5f * cosA)          (SampleTransmittanceLUT)
 *
 * Transmittance table T (TransmittanceLUT.compute:25-51), texel (x, y), one lane per texel:
 *       disc = fmaxf(0, (rad * rad) * (mu * mu - 1) + Ra * Ra);   step = fmaxf(0, (-rad) * mu + sqrtf(disc)) / 500
 *       E_c = 0;  for i = 0 .. 499:   d = ((float)i + 0.5f) * step
 *                                      sr = sqrtf((d * d + ((2 * rad) * mu) * d) + rad * rad)
 *                                      E_c = E_c + ext_c(sr - Rp) * step
 *       T[y][x] = (expf(-E_r), expf(-E_g), expf(-E_b), 0)
 * The march of a downward ray runs on through the planet, as the reference's does: the densities overflow to +inf
 * there and T = 0.
 *
 * Multiscatter table M (MultiscatteringLUT.compute:56-127), texel (x, y), one wave per texel, lane i of 64 taking the
 * reference's direction i:
 *       z = ((float)i + 0.5f) / 64;   xy = sqrtf(1 - z * z);   az = ((z * 8) * PI) * 2
 *       dir = (sinf(az) * xy, cosf(az) * xy, z)
 *       off = (-rad) * dir.y;   rc2 = rad * rad - off * off;   hit = rc2 < Rp * Rp and dir.y < 0
 *       end = hit ? off - sqrtf(Rp * Rp - rc2) : sqrtf(Ra * Ra - rc2) + off;     step = end / 32
 *       t_c = 1;  L_c = 0;  F_c = 0;  cur = step * 0.5f
 *       for j = 0 .. 31:   p = (cur * dir.x, rad + cur * dir.y, cur * dir.z);   sr = sqrtf((p.x * p.x + p.y * p.y) + p.z * p.z)
 *                          h = sr - Rp;   ins_c = (LUTAT(T, sr, mu)_c * sca_c(h)) * (1 / (4 * PI))
 *                          nt_c = t_c * expf((-ext_c(h)) * step);   ti_c = (t_c - nt_c) / ext_c(h)
 *                          L_c = L_c + ti_c * ins_c;   F_c = F_c + ti_c * sca_c(h);   cur = cur + step;   t_c = nt_c
 *       if hit:  L_c = L_c + ((t_c * LUTAT(T, rad, mu)_c) * (GA_c / PI)) * mu
 * The 64 lanes' L_c and F_c are summed by the fixed butterfly of ocean_body_buoyancy: for s = 32, 16, ..., 1:
 * a_i = a_i + a_(i xor s) for every lane i; the sum is a_0 (in numpy: fold the upper half onto the lower half until
 * one is left).  This replaces the reference's sequential sum over i, a deliberate deviation: the result depends on
 * neither the launch grid nor the scheduling.  Then
 *       M[y][x] = (L_r / (64 - F_r), L_g / (64 - F_g), L_b / (64 - F_b), 1)              (the reference's own divisor, :125)
 *
 * Sky-view table S (SkyViewLUT.compute:83-148), texel (x, y) of W x H, one lane per texel, for the unit direction
 * towards the sun (ocean_sky_update normalises `sun` on the host: len = sqrtf((x * x + y * y) + z * z), sun / len by
 * three divisions; the shader's own normalize is not repeated):
 *       lon = -PI + (((float)x + 0.5f) / ((float)W - 1)) * (2 * PI);   v = 1 - ((float)y + 0.5f) / ((float)H - 1)
 *       rad = Rp;   beta = acosf(sqrtf(rad * rad - Rp * Rp) / rad);   zha = PI - beta
 *       a = v * 2 - 1;   a = a * a;   lat = v < 0.5f ? (1 - a) * zha : zha + a * beta
 *       dir = (sinf(lon) * sinf(lat), cosf(lat), cosf(lon) * sinf(lat))
 *       cs = (dir.x * sun.x + dir.y * sun.y) + dir.z * sun.z
 *       PR = (3 / (16 * PI)) * (1 + cs * cs)
 *       PM = ((3 / (8 * PI)) * ((1 - g * g) * (1 + cs * cs))) / ((2 + g * g) * powf(fabsf((1 + g * g) - (2 * g) * cs), 1.5f))
 *       off = (-rad) * dir.y;   rc2 = rad * rad - off * off;   top = sqrtf(Ra * Ra - rc2);   start = fmaxf(0, off - top)
 *       end = (rc2 < Rp * Rp and dir.y < 0) ? off - sqrtf(Rp * Rp - rc2) : top + off;     step = (end - start) / 32
 *       t_c = 1;  L_c = 0;  cur = step * 0.5f + start
 *       for i = 0 .. 31:   p, sr, h as above
 *                          ins_c = LUTAT(T, sr, sun.y)_c * (dr * (RS_c * PR) + dm * (MS_c * PM))
 *                          ins_c = ins_c + LUTAT(M, sr, sun.y)_c * sca_c(h)
 *                          nt_c, ti_c as above;   L_c = L_c + ti_c * ins_c;   cur = cur + step;   t_c = nt_c
 *       S[y][x] = (powf(fabsf(L_r), G), powf(fabsf(L_g), G), powf(fabsf(L_b), G), 1),   G = 1.0f / 2.2f (one fp32 division)
 * The reference's quirks are kept: (id + 0.5) / (W - 1) puts the last column and the last row slightly past the end
 * (row H - 1 lies past the zenith, row 0 looks straight down), the table holds pow(|L|, 1 / 2.2), and the texels
 * whose ray ends on the planet (about the lower half of the rows) are ill-conditioned in fp32 as they are in the
 * reference (end = off - sqrtf(Rp^2 - rc2) cancels with rc2 quantised to 4e6 m^2).  They are finite.
 *
 * ocean_atmosphere queues the transmittance and then the multiscatter launch on the ctx stream.  The six sizes are
 * T's, M's and S's width and height; all six 0 selects AtmosphereController's 64 x 256, 64 x 64 and 256 x 128, otherwise
 * each lies in [2, OCEAN_ATMOSPHERE_MAX_DIM].  The tables are allocated once per context, freed and reallocated by a
 * call with other sizes, and freed by ocean_destroy.  The sky-view table is stale after every ocean_atmosphere.
 * Needs no ocean_init_spectrum.
 * ocean_sky_update queues the sky-view launch on the ctx stream, ordered with the steps and with later camera calls:
 * the per-frame call (the reference re-runs it in every Update).
 * ocean_atmosphere_read copies table `which` to the host buffer `out` of width * height * 16 bytes; blocking.
 * ocean_atmosphere_lut gives table `which`'s device pointer and size; the pointer is valid until the next
 * ocean_atmosphere with other sizes or ocean_destroy, and a reader orders itself behind the ctx stream.
 * ocean_sun_color: the colour of the sun's light, the LC a caller puts into the camera's material.  It restates
 * TurnTransmittanceIntoColorGradient (AtmosphereController.cs:129-154) and Update (:187-188) on the host in fp32, over
 * a host copy of column 0 of T, fetched (blocking) by the first call after an ocean_atmosphere and kept:
 *       for k < 8, t_k of (0.01, 0.14, 0.28, 0.36, 0.57, 0.75, 0.86, 0.99):   key_k = READ(T, 0, t_k) * 2.5f   (which is
 *            column 0: Y = fminf(fmaxf(t_k * (float)H - 0.5f, 0), (float)(H - 1)), lo + fy * (hi - lo), then * 2.5f)
 *       e = (sun.y / len + 1) * 0.5f                       ((dot(forward, down) + 1) * 0.5 with forward = -sun / len)
 *       rgb = key_0 if e <= t_0;  key_7 if e >= t_7;  else, with t_k <= e < t_(k+1):
 *             f = (e - t_k) / (t_(k+1) - t_k);   rgb_c = key_k_c + f * (key_(k+1)_c - key_k_c)
 * The reference passes the table through an 8-bit RGBA32 texture on the way (and so clamps 2.5 T to 1); this
 * library does not: a stated deviation.
 *
 * The camera sees it: ocean_camera* with mode OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT.  `bytes`, the record layout
 * and every statement of OCEAN_CAMERA_COLOR hold, except sky() and the MISS pixel; material[26..31] are ignored (but
 * still refused when not finite).  With pi the camera's own (float)3.14159265358979:
 *       SKY(r):  len = sqrtf((r.x * r.x + r.y * r.y) + r.z * r.z);   n = (r.x / len, r.y / len, r.z / len)
 *                az = atan2f(n.x, n.z);   alt = fmaxf(asinf(fminf(n.y, 1)), 0)
 *                u = (az + pi) / (2 * pi);   v = 0.5f + 0.5f * sqrtf((alt * 2) / pi)
 *                SKY_c = 2 * READ(S, u, v)_c                  (SampleSkyLUT, Atmosphere.shader:41-53; the 2 is :78)
 * The clamp of the altitude is this library's: it stands where the two-colour sky has saturate(r.y) (a reflection
 * below the horizon sees the horizon), and it keeps the lookup off the ill-conditioned rows of S.
 *   HIT:   r = ((2 * ndv) * n.x - V.x, (2 * ndv) * n.y - V.y, (2 * ndv) * n.z - V.z);   env_c = (SKY(r)_c * pi) * ke.
 *          The sun's disc is not reflected: the sun's lobes are the BRDF terms.
 *   MISS:  spot = 0 if d.y <= 0, else (SunShape, :57-63, in fp32):
 *                 q = L - d;   dist = sqrtf((q.x * q.x + q.y * q.y) + q.z * q.z);   x = clamp01(dist / SZ)
 *                 spot = 1 - (x * x) * (3 - 2 * x)
 *          colour_c = SKY(d)_c + (spot * spot) * LC_c        (L, LC of the material, SZ of the atmosphere's params)
 *   SUBMERGED stays C.
 * OCEAN_CAMERA_SKY_LUT with OCEAN_CAMERA_HITS or OCEAN_CAMERA_RANGE is OCEAN_E_INVALID_ARG; on a context whose sky-view
 * table is absent or stale the mode is OCEAN_E_STATE, after the argument checks.
 *
 * OCEAN_E_INVALID_ARG, checked before any device call and before the context wherever the context is not needed to
 * decide: a null pointer; a `params` value that is not finite; Rp <= 0 or Ra <= Rp; HR <= 0 or HM <= 0; a nonzero
 * reserved float; a size outside [2, OCEAN_ATMOSPHERE_MAX_DIM] (unless all six are 0); a `sun` that is not finite or
 * whose len is 0 or not finite; an unknown `which`; then a null context; then, of ocean_atmosphere_read, a wrong
 * `bytes` (after the state tests: the sizes are the context's).  OCEAN_E_STATE: ocean_sky_update, ocean_sun_color,
 * ocean_atmosphere_read or ocean_atmosphere_lut before ocean_atmosphere, and ocean_atmosphere_read of
 * OCEAN_LUT_SKYVIEW while it is stale.  The three launches count as kind 2 of ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_ATMOSPHERE_FLOATS 32
#define OCEAN_ATMOSPHERE_MAX_DIM 1024
#define OCEAN_LUT_TRANSMITTANCE 0
#define OCEAN_LUT_MULTISCATTER 1
#define OCEAN_LUT_SKYVIEW 2
int ocean_atmosphere(ocean_ctx *ctx, const float *params, int transmittance_width, int transmittance_height,
                     int multiscatter_width, int multiscatter_height, int skyview_width, int skyview_height);
int ocean_sky_update(ocean_ctx *ctx, const float *sun);
int ocean_atmosphere_read(ocean_ctx *ctx, int which, float *out, size_t bytes);
int ocean_atmosphere_lut(ocean_ctx *ctx, int which, void **dev, size_t *width, size_t *height);
int ocean_sun_color(ocean_ctx *ctx, const float *sun, float *rgb);

/* Spray particles: the particle system that reads the whitecap list.  ocean_whitecaps_device leaves the emitters on
 * the device; without this entry a host that wants spray lands that list, integrates its particles on the CPU,
 * uploads their positions, asks ocean_query_surface which of them fell back into the sea, lands the answers and
 * compacts the survivors, every frame and every substep: the loop ocean_body_step removed for hulls.  Here one
 * call spawns from the list, takes S substeps, retires and compacts, and a pool of particles stays on the device
 * from frame to frame.  The reference has no counterpart.
 *
 * `pool` and `out` each hold capacity + 1 records of 32 B; `bytes` must equal (capacity + 1) * 32.  Record 0 is a
 * header of eight uint32 in the whitecap list's layout: T, W, M, capacity, 0, 0, 0, 0.  Records 1 .. W are
 * particles of eight floats:
 *       [0..2] = the position p      [3] = the age a, in seconds
 *       [4..6] = the velocity v      [7] = a tag, carried bit for bit
 * An all-zero header is an empty pool.  Of the input pool's header only [1] is read, on the device, as
 * n = min(header[1], capacity).  `emitters` is NULL (no spawning; emit_capacity must be 0) or a list exactly as
 * ocean_whitecaps* writes it, of emit_capacity + 1 records, with e = min(header[1], emit_capacity).  The two clamps
 * are the kernel's guard against a header this library did not write: no record beyond `capacity` or
 * `emit_capacity` is ever read.
 *
 * `spray` is a host array of OCEAN_SPRAY_FLOATS floats in every form, read before the call returns and passed to the
 * kernel by value, like `camera`:
 *       [0] h  the substep, seconds      [1] g   gravity              [2] kd    linear drag against the wind, 1/s
 *       [3..5] wind                      [6] life  seconds            [7] jet   scale of the water's velocity at spawn
 *       [8] lift  upward speed per unit of the emitter's foam         [9..15]   reserved, must be 0
 *
 * Definition.  All arithmetic is fp32, one rounding per operation in the order written, no fused multiply-add.
 * Candidates j = 0 .. M - 1, M = n + e:
 *       j < n:   pool record 1 + j:   (p, a, v, tag) = ([0..2], [3], [4..6], [7])
 *       else:    r = emitters record 1 + (j - n):   p = r[0..2],  a = 0,  tag = r[7],
 *                v = (jet * r[4],  jet * r[5] + lift * r[3],  jet * r[6])
 * A spawned particle is stepped like the rest, from age 0.  One substep of a live candidate (semi-implicit Euler, as
 * ocean_body_step):
 *       acc = (kd * (wind.x - v.x),  kd * (wind.y - v.y) - g,  kd * (wind.z - v.z))
 *       v'  = (v.x + h * acc.x,  v.y + h * acc.y,  v.z + h * acc.z)
 *       p'  = (p.x + h * v'.x,   p.y + h * v'.y,   p.z + h * v'.z)
 *       a'  = a + h
 *       eta = rec(p'.x, p'.z)[0]        rec = OCEAN_QUERY_SURFACE's record for that point with K = `iterations`, bit for bit
 *       alive iff (p'.y > eta) and (a' < life)                 (fp32 compares: a NaN fails both and retires the particle)
 * A candidate takes S = `substeps` substeps, or stops at the first it does not survive.  Then
 *       T = the number of survivors,   rank(j) = the number of survivors j' < j,   W = min(T, capacity)
 * and every survivor with rank(j) < capacity writes record 1 + rank(j) = (p', a', v', tag) of its last substep.
 * Records W + 1 .. capacity are not written.  On overflow the first `capacity` survivors in candidate order are
 * kept, so old particles outlive new spawns, and T still counts every survivor.  S substeps in one call equal S
 * chained calls of one substep with NULL emitters after the first, bit for bit.
 * The water is the frame's, the same for all substeps, and only DISP is read.  OCEAN_F_VELOCITY is not required: a
 * context without it spawns from +0 velocities, as its whitecap list says.  DISPLACEMENT_ONLY contexts are valid
 * (they have no whitecap lists of their own: pass NULL or a list from elsewhere).
 *
 * Three launches (step, scan, emit; kind 2 of ocean_kernel_stats / ocean_kernel_name) with no atomics and no
 * workgroup that waits for another, the whitecaps' compaction: the result does not depend on the launch grid or on
 * scheduling.  Each candidate is stepped once per call.  The launch grid follows capacity + emit_capacity, M being
 * known only on the device.  Their scratch (32 B per candidate of capacity + emit_capacity, plus masks and counts)
 * belongs to the context: allocated by the first call that needs it, grown when a call needs more, freed by
 * ocean_destroy.
 * Air skip, as ocean_raycast's: with H the height no wave reaches (there), p'.y > H over a finite (p'.x, p'.z) decides
 * the first clause of `alive` true without a sample (a position whose x or z is a NaN or infinite has eta = NaN and is
 * retired as defined); every result bit is as defined above, only the time differs.  The bounds launches
 * on a context whose bounds are stale, and OCEAN_RAY_BOUNDS=0, are exactly ocean_raycast's.
 *
 * ocean_spray_step: `pool`, `emitters` and `out` are host buffers; blocks.
 * ocean_spray_step_device: they are device pointers, each 16-B aligned (else OCEAN_E_INVALID_ARG); async on the ctx
 * stream, ordered after the queued steps.  `out` may overlap neither input: ping-pong two pools.
 * ocean_spray_step_async: `pool` and `emitters` are host buffers, consumed before the call returns; `out` is a host
 * destination (pinned, ocean_host_alloc).  The pool is stepped into a readback slot on the ctx stream, after the
 * steps queued so far and before later ones, and all (capacity + 1) * 32 bytes (at most 2 MiB: every result fits a
 * slot) are copied on the copy stream, with the same ocean_readback_status / _wait / _release / _copy_ms.  The
 * inputs outgrow a slot: they are staged in a pinned block and a device block that the slot owns beside its own
 * memory, allocated by the slot's first spray request.  *req is NULL after every failure.
 * The host and async forms stage pool and list and take at most OCEAN_SPRAY_MAX_STAGED particles; the device form
 * takes OCEAN_SPRAY_MAX_PARTICLES.
 * All three: OCEAN_E_INVALID_ARG, checked before any device call and before the context wherever the context is not
 * needed: a null `spray`, `pool`, `out` or `req`; iterations outside [0, 16]; substeps outside
 * [1, OCEAN_SPRAY_MAX_SUBSTEPS]; a `spray` value that is not finite or a nonzero reserved float; capacity outside
 * [1, limit of the form]; emit_capacity outside [1, OCEAN_WHITECAP_MAX_RECORDS] when `emitters` is not NULL, or
 * nonzero when it is NULL; (capacity + emit_capacity) * substeps > 1 << 24 (in 64 bits); a wrong `bytes`; a misaligned
 * device pointer; then a null ctx and a tile out of range.  Then OCEAN_E_STATE before ocean_init_spectrum and
 * OCEAN_E_UNSUPPORTED on a column-parity context (as the queries). */
#define OCEAN_SPRAY_FLOATS 16
#define OCEAN_SPRAY_MAX_PARTICLES ((1 << 20) - 1) /* device form */
#define OCEAN_SPRAY_MAX_STAGED 65535              /* host and async forms, which stage pool and list */
#define OCEAN_SPRAY_MAX_SUBSTEPS 64
int ocean_spray_step(ocean_ctx *ctx, int tile, int iterations, int substeps, const float *spray, const float *pool,
                     int capacity, const float *emitters, int emit_capacity, float *out, size_t bytes);
int ocean_spray_step_device(ocean_ctx *ctx, int tile, int iterations, int substeps, const float *spray,
                            const float *pool, int capacity, const float *emitters, int emit_capacity, float *out,
                            size_t bytes);
int ocean_spray_step_async(ocean_ctx *ctx, int tile, int iterations, int substeps, const float *spray, const float *pool,
                           int capacity, const float *emitters, int emit_capacity, float *out, size_t bytes,
                           ocean_readback **req);

/* Camera views that see the bodies: ocean_camera* with boxes in front of the water.  ocean_body_step_device keeps the
 * hulls on the device and ocean_camera* makes pictures of the sea, but a lidar's range image shows no other vessel and
 * a picture of four thousand floating boxes shows water alone: a host that wants them lands the HITS image at 32 B
 * per pixel and the body states, intersects every pixel's ray with every box on the CPU and shades again.  Here the
 * kernel tests a pixel's ray against the bodies and against the water and keeps the nearer of the two.
 *
 * ctx, tile, mode, iterations, steps, refine, camera, material, width, height, out and bytes, the modes (HITS, RANGE,
 * COLOR, COLOR | SKY_LUT), the three forms, their ordering and the slot rule of the async form are exactly
 * ocean_camera*'s.  New:
 *   box:    float[6] = (lo.x, lo.y, lo.z, hi.x, hi.y, hi.z): one box in the body frame, before the scale, shared by
 *           all bodies as a hull is.  A host array in every form, passed to the kernel by value.
 *   paint:  float[OCEAN_BODY_PAINT_FLOATS] = (A.r, A.g, A.b, ka): the bodies' albedo and the weight of the sky's
 *           light on them.  A host array passed by value; read in the colour modes only, NULL allowed otherwise.
 *   bodies, stride, count: record b starts at bodies + b * stride floats, and its first ten floats are (c, q, s) of an
 *           ocean_body_buoyancy `bodies` record; the rest is not read.  stride in [10, 64]: 10 is a `bodies` array, 32
 *           the `out` or `state` of ocean_body_step*, which the device form takes where it lies.  count in
 *           [0, OCEAN_BODY_MAX_BODIES] in all forms.  count = 0 is valid in all forms, `bodies` may then be NULL, and
 *           the image is ocean_camera's, bit for bit.  The device form takes a device pointer, 4-B aligned; the other
 *           two a host buffer of (count - 1) * stride + 10 floats, staged and consumed before the call returns.
 *
 * All arithmetic is fp32, one rounding per operation in the order written (no fused multiply-add); sqrtf and / are
 * correctly rounded.  Per pixel, o, d, t0, t1 and R_k are ocean_camera's.  Per body, with u = (qx, qy, qz) and rot as
 * in ocean_body_step:
 *       w  = o - c (componentwise);   ob = rot(-u, qw, w);   db = rot(-u, qw, d)
 *       per axis i = x, y, z:   l = s_i * lo_i;  h = s_i * hi_i
 *           if db_i == 0:  the body is not met unless fminf(l, h) <= ob_i <= fmaxf(l, h);  then n_i = -INFINITY, f_i = +INFINITY
 *           else:          a = (l - ob_i) / db_i;  e = (h - ob_i) / db_i;  n_i = fminf(a, e);  f_i = fmaxf(a, e)
 *       tn = fmaxf(fmaxf(n_x, n_y), n_z);   tf = fminf(fminf(f_x, f_y), f_z)
 *       met  iff  tn <= tf  and  tf >= t0  and  tn <= t1          (with t1 < t0 no body is met)
 *       te = fmaxf(tn, t0)
 *       normal: if tn >= t0:  i = the first of x, y, z with n_i == tn;  nb = +0 but nb_i = (db_i > 0 ? -1 : +1);
 *                             nw = rot(u, qw, nb)
 *               else (the eye is inside the box):  nw = (-d.x, -d.y, -d.z)
 * The pixel's body is the met body of smallest te, the lowest b on ties.  The pixel is a body pixel iff a body is met
 * and R_k's status is MISS, or HIT with te < t* (t* = R_k[0]).  Water wins ties, and a SUBMERGED pixel stays
 * SUBMERGED.  Every other pixel is exactly ocean_camera's.  A body pixel is
 *   HITS:   (te, 0, 0, (float)OCEAN_RAY_BODY, nw.x, nw.y, nw.z, (float)b)
 *   RANGE:  te
 *   COLOR:  (A_c * (ka * amb_c + LC_c * fmaxf(dot(nw, L), 0)), (float)OCEAN_RAY_BODY), c = r, g, b, with
 *           amb_c = sky(nw.y)_c of the two-colour sky, or SKY(nw)_c with OCEAN_CAMERA_SKY_LUT; dot, L and LC are the
 *           camera's.
 * Limits of the feature: bodies are not reflected in the water, cast no shadow and are not fogged under the water
 * (ocean_camera_scene* below adds the three);
 * the library does not inspect records, so a non-unit quaternion distorts the box as the formulas say, and non-finite
 * values give unspecified numbers (never an access outside the textures or the records).
 * Cull and early stop.  The kernel does not test every body per pixel: per 16 x 16-pixel tile it drops the bodies
 * whose bounding sphere lies off a cone around the tile's rays or outside [t0, t1], with a derived margin, and it
 * ends a pixel's march at the first node at or behind te that is above the water, where any t* exceeds te.  Every
 * result bit is as defined above; only the time differs.  OCEAN_CAMERA_CULL=0 in the environment (read by
 * ocean_create) makes every body a survivor of the cull; the air skip, the bounds launches and OCEAN_RAY_BOUNDS=0 are
 * ocean_camera's.
 *
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for everything ocean_camera* refuses, a null `box`,
 * a null `paint` in a colour mode, a `box` value or a value of a `paint` that is passed that is not finite, stride
 * outside [10, 64], count outside [0, OCEAN_BODY_MAX_BODIES], a null `bodies` with count > 0 or a misaligned device
 * `bodies`; then OCEAN_E_STATE and OCEAN_E_UNSUPPORTED as for the camera.  The launch counts as kind 2 of
 * ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_RAY_BODY 3
#define OCEAN_BODY_PAINT_FLOATS 4
int ocean_camera_bodies(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine, const float *camera,
                        const float *material, int width, int height, const float *box, const float *paint,
                        const float *bodies, int stride, int count, float *out, size_t bytes);
int ocean_camera_bodies_device(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine,
                               const float *camera, const float *material, int width, int height, const float *box,
                               const float *paint, const float *bodies, int stride, int count, float *out, size_t bytes);
int ocean_camera_bodies_async(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine,
                              const float *camera, const float *material, int width, int height, const float *box,
                              const float *paint, const float *bodies, int stride, int count, float *out, size_t bytes,
                              ocean_readback **req);

/* Camera views in which the water sees the bodies: shadows on it, reflections in it, hulls through it.
 * ocean_camera_bodies* puts the hulls in front of the sea, but the sea does not know they are there: nothing shows
 * where a hull meets the water.  The fragment stage of Water.shader reads scene geometry in three places, which
 * ocean_camera* had to define away: shadowFactor (:357, used at :368 and :370, with _ShadowsColor and
 * _ShadowsIntensity), UnderwaterView (:143-172, with _WaterFogDensity) and EnvironmentReflections (:181-188).  Here the
 * geometry is the bodies', and the three are evaluated at every water pixel.
 *
 * Every argument but `optics` and `mode`, the three forms, their ordering and staging, the slot rule of the async form,
 * the alignment rules, the state rules and the kernel-stats kind are exactly ocean_camera_bodies*'s.  New:
 *   optics: float[OCEAN_SCENE_OPTICS_FLOATS] = (SH.r, SH.g, SH.b, SI, WF, reach): [_ShadowsColor], [_ShadowsIntensity],
 *           [_WaterFogDensity], and the length searched by the two secondary rays.  A host array in every form, passed
 *           to the kernel by value and read in every mode: never NULL.
 *   mode:   OCEAN_CAMERA_COLOR, OCEAN_CAMERA_COLOR | OCEAN_CAMERA_SKY_LUT or OCEAN_CAMERA_LINKS (valid here only).
 *           `material` is required in all three (LINKS takes L and the normal's lod from it), `paint` in the two
 *           colour modes; in LINKS mode it may be NULL.
 *   bytes:  width * height * 16 in every mode.
 *
 * All arithmetic is fp32, one rounding per operation in the order written (no fused multiply-add); sqrtf and / are
 * correctly rounded.  meet(p, r, s0, s1) is the body test of ocean_camera_bodies with o := p, d := r, t0 := s0,
 * t1 := s1: the met body of smallest te, the lowest b on ties, its te and its nw (r is used as it is, whatever its
 * length); it also serves as "any body met".  paintc(nw)_c = A_c * (ka * amb(nw)_c + LC_c * fmaxf(dot(nw, L), 0)) is
 * the body pixel's colour, amb following the sky mode.  Per pixel, o, d, t0, t1, R_k and t* are the camera's, and
 * (b1, te1, nw1) = meet(o, d, t0, t1) is ocean_camera_bodies' own test.  A body pixel, a MISS pixel and a SUBMERGED
 * pixel are exactly ocean_camera_bodies' in the colour modes.  A water HIT pixel (HIT and not a body pixel) has
 *       q = (o.x + t* * d.x, o.y + t* * d.y, o.z + t* * d.z)
 * and n, foam, eta, V, ndv, F, g, ry and the rest of the camera's "Colour of a hit".  Then
 *   through the water (UnderwaterView without the screen-space offset: the ray goes straight on):
 *       if b1 >= 0 (so te1 >= t*):  depth = te1 - t*;  fog = exp2f(-(WF * depth));
 *                                   base_c = C_c + fog * (paintc(nw1)_c - C_c)
 *       else:                       base_c = C_c
 *       refraction_c = base_c + (g * SS_c) * LC_c
 *   shadow:
 *       sf = 0 if L.y > 0 and meet(q, L, 0, reach) meets any body, else sf = 1
 *   reflection:
 *       rd = ((2 * ndv) * n.x - V.x, ry, (2 * ndv) * n.z - V.z);   (b2, te2, nw2) = meet(q, rd, 0, reach)
 *       src_c = paintc(nw2)_c if a body is met, else the camera's sky term: sky(ry)_c, or SKY(rd)_c
 *       env_c = (src_c * pi) * ke
 *   composition:
 *       sf == 1:  reflections_c and e_c are the camera's expressions, unchanged
 *       sf == 0:  reflections_c = env_c;   m_c = refraction_c + F * (reflections_c - refraction_c);
 *                 e_c = m_c + SI * (SH_c - m_c)                                                    (:370)
 *       then the foam lerp (:371) as for the camera; the fourth channel is the status.
 * A water pixel with sf == 1, b1 < 0 and b2 < 0 is therefore ocean_camera_bodies' pixel bit for bit, and so is the whole
 * image when count == 0.
 *   OCEAN_CAMERA_LINKS: out[4k + 0..3] = (sf, (float)b1t, (float)b2, (float)status) for a water HIT pixel, b1t = b1 if
 *       a body shows through the water, else -1, and b2 = -1 if no body is reflected; a body pixel is
 *       (1, (float)b, -1, (float)OCEAN_RAY_BODY); MISS and SUBMERGED pixels are (1, -1, -1, (float)status).  Every
 *       discrete decision of the colour image, and a label image: which hull a pixel's shadow and reflection belong to.
 * Limits of the feature: shadows are hard (a point sun); bodies do not shadow or reflect each other; the colours seen
 * through the water or in it are unshadowed; a hull behind a wave crest is fogged by its distance behind the surface,
 * as the shader's depth difference does; `reach` bounds both secondary rays; exp2f is a third operation, beside powf
 * and the sky table's atan2f and asinf, whose last bits belong to the device's math library.
 * Culls.  The primary cull and the early stop are ocean_camera_bodies'.  For the secondary rays the kernel drops, per
 * 16 x 16-pixel tile, the bodies whose bounding sphere is further than `reach` from the bounding box of the tile's
 * points q, with a derived margin.  Every result bit is as defined above; only the time differs, and it grows with
 * `reach`.  OCEAN_CAMERA_CULL=0 makes every body a survivor of both culls.
 *
 * All three: OCEAN_E_INVALID_ARG, checked before any device call, for a null `optics`, an `optics` value that is not
 * finite, reach < 0, the modes OCEAN_CAMERA_HITS and OCEAN_CAMERA_RANGE (ocean_camera_bodies* serves them) and every
 * other mode not named above, a null `material`, a null `paint` in a colour mode, and everything
 * ocean_camera_bodies* refuses; then OCEAN_E_STATE and OCEAN_E_UNSUPPORTED as for the camera.  The launch counts as
 * kind 2 of ocean_kernel_stats / ocean_kernel_name. */
#define OCEAN_CAMERA_LINKS 3 /* valid only in ocean_camera_scene* */
#define OCEAN_SCENE_OPTICS_FLOATS 6
int ocean_camera_scene(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine, const float *camera,
                       const float *material, int width, int height, const float *box, const float *paint,
                       const float *optics, const float *bodies, int stride, int count, float *out, size_t bytes);
int ocean_camera_scene_device(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine,
                              const float *camera, const float *material, int width, int height, const float *box,
                              const float *paint, const float *optics, const float *bodies, int stride, int count,
                              float *out, size_t bytes);
int ocean_camera_scene_async(ocean_ctx *ctx, int tile, int mode, int iterations, int steps, int refine,
                             const float *camera, const float *material, int width, int height, const float *box,
                             const float *paint, const float *optics, const float *bodies, int stride, int count,
                             float *out, size_t bytes, ocean_readback **req);

/* Readback timing (off after ocean_create): while on, each new ocean_read_async /
 * ocean_read_height_async / ocean_query_surface_async / ocean_surface_grid_async /
 * ocean_body_buoyancy_async / ocean_query_velocity_async / ocean_raycast_async / ocean_body_dynamics_async /
 * ocean_whitecaps_async / ocean_camera_async / ocean_body_step_async / ocean_spray_step_async /
 * ocean_camera_bodies_async / ocean_camera_scene_async request records HIP
 * timing events around its device-to-host copy, for ocean_readback_copy_ms.  Requests made while it is off record only untimed events. */
int ocean_set_readback_timing(ocean_ctx *ctx, int enable);

/* Duration of a completed request's device-to-host copy in ms (HIP events on the copy stream around
 * the copy itself: the link's share of the request, without the wait for the queued frames or the
 * on-device snapshot).  OCEAN_E_STATE while the request is pending, or if it was made with readback
 * timing off.  No reference counterpart: AsyncGPUReadback exposes no timing; hosts use it to
 * attribute a readback-bound loop. */
int ocean_readback_copy_ms(ocean_readback *rb, float *ms);

/* Pinned host memory for ocean_read_async destinations (hipHostMalloc). */
int ocean_host_alloc(size_t bytes, void **out);
void ocean_host_free(void *p);

/* Thread-local message describing the last failure on this thread ("" if none). */
const char *ocean_last_error(void);

/* OCEAN_ABI_VERSION of the loaded library. */
int ocean_abi_version(void);

#ifdef __cplusplus
}
#endif
#endif /* OCEAN_OCEAN_H */
