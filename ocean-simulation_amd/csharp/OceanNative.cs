// P/Invoke binding of liboceanhip.so (include/ocean/ocean.h) for the reference's
// C# host (Unity / Mono / .NET).  Compile-ready; not built in this repository's CI
// (no C# toolchain in the build image).  Every struct is blittable and laid out
// exactly as the C declaration; every call returns OceanStatus (0 = OK).
using System;
using System.Runtime.InteropServices;

namespace OceanHip
{
    public enum OceanStatus : int
    {
        Ok = 0,
        InvalidArg = -1,
        Unsupported = -2,
        State = -3,
        Device = -4,
        OutOfMemory = -5,
    }

    [Flags]
    public enum OceanFlags : uint
    {
        None = 0,
        DisplacementOnly = 0x1,  // 2 planes -> DISP only
        Normals = 0x2,           // also write the per-cascade NORMAL texture
        Unfused = 0x4,           // reference-shaped schedule: evolve -> 4 x IFFT -> fill
        Mips = 0x8,              // DERIV / TURB mip chains regenerated every step (GenerateMips)
        Velocity = 0x10,         // also keep the VELOCITY texture (d/dt of the displacement), written every step
    }

    public enum OceanTexture : int
    {
        Noise = 0, H0 = 1, Waves = 2,
        Plane0 = 3, Plane1 = 4, Plane2 = 5, Plane3 = 6,   // DxDz, DyDxz, DyxDyz, DxxDzz
        Displacement = 7, Derivatives = 8, Turbulence = 9, Normal = 10,
        Velocity = 11,   // OceanFlags.Velocity contexts only: d/dt of Displacement.xyz, dDxz/dt in .w
    }

    // WaterBody.cs:10-14
    [StructLayout(LayoutKind.Sequential)]
    public struct OceanParams
    {
        public float windSpeed, windDirX, windDirY, gravity, fetch, depth;
    }

    // WaterCascade.cs:10-24
    [StructLayout(LayoutKind.Sequential)]
    public struct OceanCascade
    {
        public float wavelength, cutoffLow, cutoffHigh, swell, fade;
    }

    public static class OceanNative
    {
        public const int AbiVersion = 4;  // OCEAN_ABI_VERSION of the header this binding follows
        const string Lib = "oceanhip";  // liboceanhip.so next to the managed assembly / on LD_LIBRARY_PATH

        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_create(int device, int n, int nCascades, int nTiles, OceanFlags flags, out IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern void ocean_destroy(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_params(IntPtr ctx, ref OceanParams p, [In] OceanCascade[] cascades);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_noise(IntPtr ctx, int tile, [In] float[] rg);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_generate_noise(IntPtr ctx, ulong seed);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_generate_noise_device(IntPtr ctx, ulong seed);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_init_spectrum(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_reset_foam(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_step(IntPtr ctx, float time);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_evolve(IntPtr ctx, float time);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_ifft2d(IntPtr ctx, int planeMask);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_fill(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_read(IntPtr ctx, OceanTexture tex, int tile, int cascade, [Out] float[] dst, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_write(IntPtr ctx, OceanTexture tex, int tile, int cascade, [In] float[] src, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_get_device_ptr(IntPtr ctx, OceanTexture tex, out IntPtr ptr, out UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_get_stream(IntPtr ctx, out IntPtr stream);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_synchronize(IntPtr ctx);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_kernel_timing(IntPtr ctx, int enable);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_kernel_stats(IntPtr ctx, int kind, out double totalMs, out long launches);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_kernel_name(IntPtr ctx, int kind, [Out] byte[] buf, UIntPtr len);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_step_bytes(IntPtr ctx, out ulong passA, out ulong passB);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_column_band(IntPtr ctx, int xBegin, int xCount);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_column_parity(IntPtr ctx, int parity);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_read_mip(IntPtr ctx, OceanTexture tex, int tile, int cascade, int level, [Out] float[] dst, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_get_mip_ptr(IntPtr ctx, OceanTexture tex, int level, out IntPtr ptr, out UIntPtr sliceStride);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_sample_world(IntPtr ctx, int tile, [In] float[] points, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_sample_world_device(IntPtr ctx, int tile, IntPtr points, int count, IntPtr output);
        // Surface queries (added within ABI 4: a host that must run on an older version-4 library catches
        // EntryPointNotFoundException on the first call).  mode: QueryReference / QuerySurface; 8 floats per point.
        public const int QueryReference = 0, QuerySurface = 1, QueryMaxPoints = 65536;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_surface(IntPtr ctx, int tile, int mode, int iterations, [In] float[] points, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_surface_device(IntPtr ctx, int tile, int mode, int iterations, IntPtr points, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_surface_async(IntPtr ctx, int tile, int mode, int iterations, [In] float[] points, int count, IntPtr dst, out IntPtr request);
        // Surface grids (added within ABI 4 in the same way).  Node (i, j) lies at (x0 + i dx, z0 + j dz), result j * nx + i;
        // mode: GridVertices / GridSurface (8 floats per node, bytes = nx * ny * 32) / GridHeightfield (1 float, nx * ny * 4).
        public const int GridVertices = 0, GridSurface = 1, GridHeightfield = 2, GridMaxNodes = 1 << 22;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_surface_grid(IntPtr ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx, float dz, int nx, int ny, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_surface_grid_device(IntPtr ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx, float dz, int nx, int ny, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_surface_grid_async(IntPtr ctx, int tile, int mode, int iterations, float lod, float x0, float z0, float dx, float dz, int nx, int ny, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Buoyant bodies (added within ABI 4 in the same way).  hull [probes][5] = (rx, ry, rz, h, v), bodies [count][10] =
        // (origin, quaternion xyzw, scale), 8 floats per body; mode and iterations as the queries (QueryReference: 0).
        public const int BodyMaxBodies = 8192, BodyMaxProbes = 4096, BodyMaxSamples = 1 << 22;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_buoyancy(IntPtr ctx, int tile, int mode, int iterations, [In] float[] hull, int probes, [In] float[] bodies, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_buoyancy_device(IntPtr ctx, int tile, int mode, int iterations, IntPtr hull, int probes, IntPtr bodies, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_buoyancy_async(IntPtr ctx, int tile, int mode, int iterations, [In] float[] hull, int probes, [In] float[] bodies, int count, IntPtr dst, out IntPtr request);
        // Body dynamics (added within ABI 4 in the same way; OceanFlags.Velocity contexts).  hull and bodies as the buoyant
        // bodies, motion [count][6] = (world linear velocity of the origin, world angular velocity); 16 floats per body:
        // the buoyancy record, then sum F xyz, sum T xyz about the origin, the largest relative speed over the wet
        // probes, the number of wet probes.  law: F = g u (DragLinear) or g |u| u (DragQuadratic) per probe.
        public const int DragLinear = 0, DragQuadratic = 1;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_dynamics(IntPtr ctx, int tile, int mode, int iterations, int law, [In] float[] hull, int probes, [In] float[] bodies, [In] float[] motion, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_dynamics_device(IntPtr ctx, int tile, int mode, int iterations, int law, IntPtr hull, int probes, IntPtr bodies, IntPtr motion, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_dynamics_async(IntPtr ctx, int tile, int mode, int iterations, int law, [In] float[] hull, int probes, [In] float[] bodies, [In] float[] motion, int count, IntPtr dst, out IntPtr request);
        // Body steps (added within ABI 4 in the same way; OceanFlags.Velocity contexts).  `substeps` substeps of the rigid
        // bodies in one launch: step [8] = (h, g, B, kd, kt, la, aa, 0), a host array in every form; props [count][4] =
        // (1 / mass, 1 / Ix, 1 / Iy, 1 / Iz); state and output [count][32] = (bodies' 10, motion's 6, then the dynamics
        // record of the last substep, ignored on input): the output of one call is the state of the next, and the
        // _device form may be given output == state.
        public const int BodyStepFloats = 8, BodyMaxSubsteps = 64, BodyStepMaxSamples = 1 << 24;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_step(IntPtr ctx, int tile, int mode, int iterations, int law, int substeps, [In] float[] step, [In] float[] hull, int probes, [In] float[] props, [In] float[] state, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_step_device(IntPtr ctx, int tile, int mode, int iterations, int law, int substeps, [In] float[] step, IntPtr hull, int probes, IntPtr props, IntPtr state, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_step_async(IntPtr ctx, int tile, int mode, int iterations, int law, int substeps, [In] float[] step, [In] float[] hull, int probes, [In] float[] props, [In] float[] state, int count, IntPtr dst, out IntPtr request);
        // Surface velocity (added within ABI 4 in the same way; OceanFlags.Velocity contexts).  8 floats per point: velocity
        // x, y, z of the water particle on the surface above the point, residual, height, p.x, p.z, dDxz/dt.
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_velocity(IntPtr ctx, int tile, int iterations, [In] float[] points, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_velocity_device(IntPtr ctx, int tile, int iterations, IntPtr points, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_query_velocity_async(IntPtr ctx, int tile, int iterations, [In] float[] points, int count, IntPtr dst, out IntPtr request);
        // Surface bounds (added within ABI 4 in the same way).  8 floats per cascade: min x, y, z, w, max x, y, z, w of
        // the displacement slice; bytes = cascades * 32.
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_surface_bounds(IntPtr ctx, int tile, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_surface_bounds_device(IntPtr ctx, int tile, IntPtr output, UIntPtr bytes);
        // Ray casts (added within ABI 4 in the same way).  8 floats per ray in (origin, direction, t0, t1) and out
        // (t*, height over the water, residual, status, normal x, y, z, foam).
        public const int RayMiss = 0, RayHit = 1, RaySubmerged = 2;
        public const int RayMaxRays = 16384, RayMaxSteps = 1024, RayMaxSamples = 1 << 24;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_raycast(IntPtr ctx, int tile, int iterations, int steps, int refine, [In] float[] rays, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_raycast_device(IntPtr ctx, int tile, int iterations, int steps, int refine, IntPtr rays, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_raycast_async(IntPtr ctx, int tile, int iterations, int steps, int refine, [In] float[] rays, int count, IntPtr dst, out IntPtr request);
        // Whitecap emitters (added within ABI 4 in the same way).  The nodes (i, j) at (x0 + i dx, z0 + j dz) whose foam at
        // `lod` is >= threshold, compacted in ascending k = j * nx + i: capacity + 1 records of 32 B, bytes = (capacity + 1) * 32.
        // Record 0 = eight uint (T selected, W = min(T, capacity) written, nx * ny, capacity, 0, 0, 0, 0); then 8 floats per
        // node: displaced x, y, z, foam, the water's velocity x, y, z (OceanFlags.Velocity contexts, else 0), (float)k.
        public const int WhitecapMaxRecords = 65535;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_whitecaps(IntPtr ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz, int nx, int ny, int capacity, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_whitecaps_device(IntPtr ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz, int nx, int ny, int capacity, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_whitecaps_async(IntPtr ctx, int tile, float lod, float threshold, float x0, float z0, float dx, float dz, int nx, int ny, int capacity, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Spray particles (added within ABI 4 in the same way).  pool and output = capacity + 1 records of 32 B, bytes =
        // (capacity + 1) * 32: record 0 = eight uint (T survivors, W = min(T, capacity) written, M candidates, capacity, 0, 0,
        // 0, 0), then 8 floats per particle: position x, y, z, age, velocity x, y, z, tag.  emitters = a whitecap list of
        // emitCapacity + 1 records, or null with emitCapacity 0.  spray = 16 floats (h, g, kd, wind x, y, z, life, jet, lift,
        // zeros).  The host and async forms take SprayMaxStaged particles, the device form SprayMaxParticles.
        public const int SprayFloats = 16;
        public const int SprayMaxParticles = (1 << 20) - 1;
        public const int SprayMaxStaged = 65535;
        public const int SprayMaxSubsteps = 64;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_spray_step(IntPtr ctx, int tile, int iterations, int substeps, [In] float[] spray, [In] float[] pool, int capacity, [In] float[] emitters, int emitCapacity, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_spray_step_device(IntPtr ctx, int tile, int iterations, int substeps, [In] float[] spray, IntPtr pool, int capacity, IntPtr emitters, int emitCapacity, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_spray_step_async(IntPtr ctx, int tile, int iterations, int substeps, [In] float[] spray, [In] float[] pool, int capacity, [In] float[] emitters, int emitCapacity, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Camera views (added within ABI 4 in the same way).  camera = 14 floats (eye, the direction through pixel (0, 0),
        // its change per column and per row, t0, t1); pixel (i, j) is element j * width + i.  CameraHits: ocean_raycast's 8
        // floats per pixel; CameraRange: the distance along the ray, +infinity after a miss, 1 float; CameraColor: r, g, b,
        // status, 4 floats, shaded with the 32 floats of `material` (ocean.h names them; null in the other two modes).
        // bytes = width * height * 32, 4 or 16.
        public const int CameraHits = 0, CameraRange = 1, CameraColor = 2;
        public const int CameraFloats = 14, CameraMaterialFloats = 32;
        public const int CameraMaxPixels = 1 << 22, CameraMaxSamples = 1 << 28;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_device(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_async(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Camera views that see the bodies (added within ABI 4 in the same way): ocean_camera with boxes in front of the
        // water.  box = 6 floats (lo, hi) in the body frame before the scale, shared by all bodies; paint = 4 floats (r, g, b,
        // ka), null outside the colour modes; record b starts at bodies + b * stride floats, its first ten floats (c, q, s),
        // stride in [10, 64] (32: the records of ocean_body_step), count in [0, BodyMaxBodies].  A body pixel has the
        // status RayBody.
        public const int RayBody = 3, BodyPaintFloats = 4;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_bodies(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, [In] float[] bodies, int stride, int count, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_bodies_device(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, IntPtr bodies, int stride, int count, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_bodies_async(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, [In] float[] bodies, int stride, int count, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Camera views in which the water sees the bodies (added within ABI 4 in the same way): ocean_camera_bodies with the
        // bodies' shadows on the water, their reflections in it and their submerged parts through it.  optics = 6 floats
        // (shadow colour r, g, b, shadow intensity, water fog density, reach of the secondary rays); mode CameraColor,
        // CameraColor | CameraSkyLut or CameraLinks (valid here only: per pixel lit or not, the body seen through the water,
        // the body reflected, the status); 16 bytes per pixel in every mode; material required, paint in the colour modes.
        public const int CameraLinks = 3, SceneOpticsFloats = 6;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_scene(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, [In] float[] optics, [In] float[] bodies, int stride, int count, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_scene_device(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, [In] float[] optics, IntPtr bodies, int stride, int count, IntPtr output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_camera_scene_async(IntPtr ctx, int tile, int mode, int iterations, int steps, int refine, [In] float[] camera, [In] float[] material, int width, int height, [In] float[] box, [In] float[] paint, [In] float[] optics, [In] float[] bodies, int stride, int count, IntPtr dst, UIntPtr bytes, out IntPtr request);
        // Mesh hulls (added within ABI 4 in the same way): the hydrostatic pressure over the wetted triangles of a mesh
        // shared by the bodies.  vertices [nverts][3] in the body frame, triangles int [ntris][3] wound counter-clockwise
        // seen from outside (the header declares them `const void *`: pass the address of a pinned int[]), bodies
        // [count][10] as the buoyant bodies; 16 floats per body: sum F xyz, wetted area, sum Tq xyz about the origin, worst
        // residual, the wetted area's first moment xyz, wet triangles, draught, wet vertices, sum Av.y, 0.  Always in
        // surface mode.
        public const int HullMaxVertices = 2048, HullMaxTriangles = 4096, HullRecordFloats = 16;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_hydrostatics(IntPtr ctx, int tile, int iterations, [In] float[] vertices, int nverts, IntPtr triangles, int ntris, [In] float[] bodies, int count, [Out] float[] output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_hydrostatics_device(IntPtr ctx, int tile, int iterations, IntPtr vertices, int nverts, IntPtr triangles, int ntris, IntPtr bodies, int count, IntPtr output);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_body_hydrostatics_async(IntPtr ctx, int tile, int iterations, [In] float[] vertices, int nverts, IntPtr triangles, int ntris, [In] float[] bodies, int count, IntPtr dst, out IntPtr request);
        // The atmosphere (added within ABI 4 in the same way; ocean.h "The atmosphere"): the three look-up tables of
        // AtmosphereController.cs, owned by the context.  `parameters` = 32 floats (ocean.h names them); the six sizes all 0
        // select the reference's.  ocean_sky_update is the per-frame call; CameraColor | CameraSkyLut then shades the
        // camera's colour image with the sky-view table, and ocean_sun_color gives the light's colour for a material.
        public const int AtmosphereFloats = 32, AtmosphereMaxDim = 1024, CameraSkyLut = 16;
        public const int LutTransmittance = 0, LutMultiscatter = 1, LutSkyView = 2;
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_atmosphere(IntPtr ctx, [In] float[] parameters, int transmittanceWidth, int transmittanceHeight, int multiscatterWidth, int multiscatterHeight, int skyviewWidth, int skyviewHeight);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_sky_update(IntPtr ctx, [In] float[] sun);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_atmosphere_read(IntPtr ctx, int which, [Out] float[] output, UIntPtr bytes);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_atmosphere_lut(IntPtr ctx, int which, out IntPtr dev, out UIntPtr width, out UIntPtr height);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_sun_color(IntPtr ctx, [In] float[] sun, [Out] float[] rgb);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_read_async(IntPtr ctx, OceanTexture tex, int tile, int cascade, IntPtr dst, UIntPtr bytes, out IntPtr request);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int ocean_readback_status(IntPtr request);   // 1 done, 0 pending, < 0 error (hasError)
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_readback_wait(IntPtr request);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern void ocean_readback_release(IntPtr request);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_readback_copy_ms(IntPtr request, out float ms);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_read_height_async(IntPtr ctx, int tile, int cascade, IntPtr dst, UIntPtr bytes, out IntPtr request);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_set_readback_timing(IntPtr ctx, int enable);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern OceanStatus ocean_host_alloc(UIntPtr bytes, out IntPtr ptr);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern void ocean_host_free(IntPtr ptr);
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        static extern IntPtr ocean_last_error();
        [DllImport(Lib, CallingConvention = CallingConvention.Cdecl)]
        public static extern int ocean_abi_version();

        public static string LastError() => Marshal.PtrToStringAnsi(ocean_last_error()) ?? "";

        public static void Check(OceanStatus s, string where)
        {
            if (s != OceanStatus.Ok) throw new InvalidOperationException($"{where} failed ({s}): {LastError()}");
        }
    }
}
