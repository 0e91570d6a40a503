// WaterBody-shaped facade over liboceanhip.so: the same public surface as
// Assets/Scripts/Water/WaterBody.cs (fields :10-33, CalculateWavesTexturesAtTime
// :180, GetWaterHeight :195, Awake :211, Update :284, OnDisable :300), with the
// GPU work done by the MI355X library instead of ComputeShader.Dispatch.
// Engine-free (no UnityEngine types) so it also runs in a plain .NET host; a
// Unity MonoBehaviour can own one of these and forward its lifecycle calls.
// Compile-ready; not built here (no C# toolchain in the build image).
using System;

namespace OceanHip
{
    public sealed class WaterCascadeDesc  // WaterCascade.cs:10-24
    {
        public float wavelength = 10.0f, cutoffHigh = 5.0f, cutoffLow = 0.0001f, swell = 0.4f, fade = 0.1f;
    }

    // What Update reads back every frame (ocean.h ocean_read_height_async): the height channel alone,
    // all GetWaterHeight reads (the reference's buoyancyData is private, WaterBody.cs:58, and .g is its
    // only use, :208), or the whole RGBA displacement slice as the reference requests it.
    // Probes reads no slice back: Update issues one ocean_query_surface_async per frame for the world positions
    // given to SetProbes (one per buoyant body) and ProbeHeights is the newest landed answer, 32 B per probe over
    // the link.  In that mode GetWaterHeight keeps returning 0, as the reference does before its first readback,
    // and buoyancyData stays empty.
    public enum Readback { Height, Rgba, Probes }

    public sealed class WaterBodyNative : IDisposable
    {
        // Ocean parameters (WaterBody.cs:10-14) and texture size (:29)
        public float windSpeed = 1.0f;
        public float windDirectionX = 1.0f, windDirectionY = 1.0f;
        public float gravity = 9.81f;
        public float fetch = 1.0f;
        public float depth = 4.0f;
        public int texturesSize = 256;
        public WaterCascadeDesc[] cascades = { new WaterCascadeDesc() };
        public int device = 0;
        public ulong seed = 20251121;   // the reference's UnityEngine.Random is unseeded; this library's generator is
        public Readback readback = Readback.Height;  // set before Awake
        public int probeMode = OceanNative.QuerySurface;  // Readback.Probes: ocean_query_surface_async's mode ...
        public int probeIterations = 4;                   // ... and fixed-point steps (0 with QueryReference)
        public bool velocity = false;   // set before Awake: also keep the VELOCITY texture (GetWaterVelocity)
        public int probeCapacity = 64;  // probes the pinned ring is sized for at Awake (or the probes set by then, if more)

        IntPtr ctx = IntPtr.Zero;
        float[] buoyancyData;           // displacement slice 0 (WaterBody.cs:58, :295): [y][x] heights, or RGBA [y][x][4]
        float[] probes = new float[0];  // SetProbes' (world x, world z) pairs
        float[] probeResults;           // the newest landed query, [M][8]
        int probeCap;
        // floats of one ring slot: a readback slice, or probeCap query results
        int Floats => readback == Readback.Probes ? probeCap * 8
                                                  : texturesSize * texturesSize * (readback == Readback.Height ? 1 : 4);

        public void Awake()
        {
            // the rules this facade relies on (ocean.h: ABI 4, no call moves the caller's current device)
            if (OceanNative.ocean_abi_version() != OceanNative.AbiVersion)
                throw new InvalidOperationException("liboceanhip ABI " + OceanNative.ocean_abi_version() + ", expected " +
                                                    OceanNative.AbiVersion);
            var flags = OceanFlags.Mips | (velocity ? OceanFlags.Velocity : OceanFlags.None);
            OceanNative.Check(OceanNative.ocean_create(device, texturesSize, cascades.Length, 1, flags, out ctx), "ocean_create");
            ApplyParams();
            OceanNative.Check(OceanNative.ocean_generate_noise(ctx, seed), "ocean_generate_noise");
            OceanNative.Check(OceanNative.ocean_init_spectrum(ctx), "ocean_init_spectrum");
            probeCap = Math.Max(Math.Max(probeCapacity, probes.Length / 2), 1);
            if (readback == Readback.Probes && probeCap > OceanNative.QueryMaxPoints)
                throw new InvalidOperationException("at most OceanNative.QueryMaxPoints probes");
            // readback ring: MaxReadbacksInFlight pinned slices allocated once, reused by every
            // request and freed only in Dispose (hipHostFree synchronizes the device: a free per
            // request would make each Update wait for the frame it just queued)
            int bytes = Floats * sizeof(float);
            for (int i = 0; i < MaxReadbacksInFlight; i++)
            {
                OceanNative.Check(OceanNative.ocean_host_alloc((UIntPtr)bytes, out var b), "ocean_host_alloc");
                ring.Add(b);
                idle.Push(b);
            }
        }

        void ApplyParams()
        {
            var p = new OceanParams { windSpeed = windSpeed, windDirX = windDirectionX, windDirY = windDirectionY,
                                      gravity = gravity, fetch = fetch, depth = depth };
            var cs = new OceanCascade[cascades.Length];
            for (int i = 0; i < cascades.Length; i++)
                cs[i] = new OceanCascade { wavelength = cascades[i].wavelength, cutoffLow = cascades[i].cutoffLow,
                                           cutoffHigh = cascades[i].cutoffHigh, swell = cascades[i].swell,
                                           fade = cascades[i].fade };
            OceanNative.Check(OceanNative.ocean_set_params(ctx, ref p, cs), "ocean_set_params");
        }

        // The commented OnValidate of WaterBody.cs:324-337: parameter change -> spectrum re-init
        // (the foam accumulator carries over, as there).
        public void OnValidate()
        {
            if (ctx == IntPtr.Zero) return;
            ApplyParams();
            OceanNative.Check(OceanNative.ocean_init_spectrum(ctx), "ocean_init_spectrum");
        }

        public void CalculateWavesTexturesAtTime(float time) =>
            OceanNative.Check(OceanNative.ocean_step(ctx, time), "ocean_step");

        // WaterBody.Update (:284-297): step, then issue a new asynchronous request of the
        // displacement slice 0 EVERY frame (AsyncGPUReadback.Request, :288); requests
        // complete in order and each completed one refreshes buoyancyData, as the
        // reference's callback does (:292-295).  Requests land in slots of a pinned ring.
        const int MaxReadbacksInFlight = 4;  // ring slots; the reference's request queue is engine-managed.
                                             // 2-4 in flight keep the 16 MiB copies back to back beside the
                                             // frames; 8 stretch each copy 2.5x (DESIGN.md section 1)
        readonly System.Collections.Generic.Queue<(IntPtr req, IntPtr buf, int count)> readbacks =
            new System.Collections.Generic.Queue<(IntPtr req, IntPtr buf, int count)>();  // count: Probes, the points asked
        readonly System.Collections.Generic.List<IntPtr> ring = new System.Collections.Generic.List<IntPtr>();
        readonly System.Collections.Generic.Stack<IntPtr> idle = new System.Collections.Generic.Stack<IntPtr>();

        void Complete((IntPtr req, IntPtr buf, int count) r, bool wait)
        {
            int n = Floats;
            int st = wait ? (OceanNative.ocean_readback_wait(r.req) == OceanStatus.Ok ? 1 : -1)
                          : OceanNative.ocean_readback_status(r.req);
            if (st == 1 && readback == Readback.Probes)
            {
                probeResults = new float[r.count * 8];
                System.Runtime.InteropServices.Marshal.Copy(r.buf, probeResults, 0, r.count * 8);
            }
            else if (st == 1)
            {
                buoyancyData ??= new float[n];
                System.Runtime.InteropServices.Marshal.Copy(r.buf, buoyancyData, 0, n);
            }                                              // st < 0: request.hasError, data dropped
            OceanNative.ocean_readback_release(r.req);
            idle.Push(r.buf);                              // slot back to the ring
        }

        public void Update(float time)
        {
            CalculateWavesTexturesAtTime(time);
            while (readbacks.Count > 0 && OceanNative.ocean_readback_status(readbacks.Peek().req) != 0)
                Complete(readbacks.Dequeue(), false);
            if (readback == Readback.Probes && probes.Length == 0) return;  // nobody asks: no request
            if (idle.Count == 0) Complete(readbacks.Dequeue(), true);  // every slot in flight: wait for the oldest
            var buf = idle.Pop();
            var bytes = (UIntPtr)(Floats * sizeof(float));
            IntPtr req;
            int count = probes.Length / 2;
            // Probes: one query for every probe, in place of the slice request: 32 B per probe come back
            var st = readback == Readback.Probes
                         ? OceanNative.ocean_query_surface_async(ctx, 0, probeMode, probeIterations, probes, count, buf, out req)
                     : readback == Readback.Height
                         ? OceanNative.ocean_read_height_async(ctx, 0, 0, buf, bytes, out req)
                         : OceanNative.ocean_read_async(ctx, OceanTexture.Displacement, 0, 0, buf, bytes, out req);
            if (st != OceanStatus.Ok) { idle.Push(buf); OceanNative.Check(st, "readback request"); }
            readbacks.Enqueue((req, buf, count));
        }

        public void WaitForReadbacks()
        {
            while (readbacks.Count > 0) Complete(readbacks.Dequeue(), true);
        }

        // WaterBody.cs:195-209, including the mapping over [-texturesSize/2, texturesSize/2].
        public float GetWaterHeight(float worldX, float worldZ)
        {
            if (buoyancyData == null) return 0f;
            float InverseLerp(float a, float b, float v) => a == b ? 0f : Math.Clamp((v - a) / (b - a), 0f, 1f);
            float u = InverseLerp(-texturesSize / 2, texturesSize / 2, worldX);
            float v = InverseLerp(-texturesSize / 2, texturesSize / 2, worldZ);
            int x = Math.Clamp((int)(u * texturesSize), 0, texturesSize - 1);
            int y = Math.Clamp((int)(v * texturesSize), 0, texturesSize - 1);
            int t = y * texturesSize + x;
            return readback == Readback.Height ? buoyancyData[t] : buoyancyData[t * 4 + 1];  // .g = Dy
        }

        // The world positions Update asks about with Readback.Probes: [M][3] (x, y, z; x and z are used, as
        // GetWaterHeight uses its worldPosition).  After Awake, at most the capacity the ring was sized for.
        // Takes effect at the next Update; answers already in flight keep their own M.
        public void SetProbes(float[] xyz)
        {
            if (ctx != IntPtr.Zero && readback == Readback.Probes && xyz.Length / 3 > probeCap)
                throw new InvalidOperationException("more probes than the capacity the ring was sized for at Awake");
            var p = new float[xyz.Length / 3 * 2];
            for (int i = 0; i < xyz.Length / 3; i++) { p[2 * i] = xyz[3 * i]; p[2 * i + 1] = xyz[3 * i + 2]; }
            probes = p;
        }

        // The newest landed query, [M][8] as ocean_query_surface returns it, or null before the first lands.
        public float[] ProbeResults() => probeResults == null ? null : (float[])probeResults.Clone();

        // The newest landed heights, [M] in SetProbes' order, or null before the first lands.
        public float[] ProbeHeights()
        {
            if (probeResults == null) return null;
            var h = new float[probeResults.Length / 8];
            for (int i = 0; i < h.Length; i++) h[i] = probeResults[i * 8];
            return h;
        }

        // What Water.shader reads at world positions (Water.shader:314-348): points are
        // (x, z, lod) triples; per point 12 floats: summed displacement + turbulence,
        // summed derivatives, normal (ocean.h ocean_sample_world).
        public float[] SampleWorld(float[] points)
        {
            var output = new float[points.Length / 3 * 12];
            OceanNative.Check(OceanNative.ocean_sample_world(ctx, 0, points, points.Length / 3, output), "ocean_sample_world");
            return output;
        }

        // The surface over a regular grid (ocean.h ocean_surface_grid): node (i, j) at (x0 + i dx, z0 + j dz) is element
        // j * nx + i of the result.  GridVertices (iterations 0, `lod` as SampleWorld): 8 floats per node, the displaced
        // vertex x, y, z, the foam, the normal, 0: MeshGenerator's plane through the domain stage of Water.shader;
        // GridSurface: ocean_query_surface's record at every node; GridHeightfield: its height alone, 1 float per node.
        public float[] SurfaceGrid(float x0, float z0, float dx, float dz, int nx, int ny, int mode = OceanNative.GridSurface,
                                   int iterations = 4, float lod = 0f)
        {
            int per = mode == OceanNative.GridHeightfield ? 1 : 8;
            // (a size outside the limits is refused by the library; no managed buffer of that size first)
            bool valid = nx >= 1 && ny >= 1 && (long)nx * ny <= OceanNative.GridMaxNodes;
            var output = new float[valid ? nx * ny * per : 0];
            OceanNative.Check(OceanNative.ocean_surface_grid(ctx, 0, mode, mode == OceanNative.GridVertices ? 0 : iterations, lod,
                                                             x0, z0, dx, dz, nx, ny, output,
                                                             (UIntPtr)(ulong)(output.Length * 4)), "ocean_surface_grid");
            return output;
        }

        // BuoyantObject.FixedUpdate's lookup for M bodies of P probes each (ocean.h ocean_body_buoyancy): hull is
        // [P][5] = (cell centre in the body frame, vertical extent, volume), bodies [M][10] = (origin, body -> world
        // quaternion xyzw, per-axis scale); per body 8 floats: submerged volume V, V * centroid relative to the
        // origin, V-weighted water normal, worst residual.  Force rho g V along +y; torque rho g (-out[3], 0, out[1]).
        public float[] Buoyancy(float[] hull, float[] bodies, int iterations = 4, int mode = OceanNative.QuerySurface)
        {
            var output = new float[bodies.Length / 10 * 8];
            OceanNative.Check(OceanNative.ocean_body_buoyancy(ctx, 0, mode, iterations, hull, hull.Length / 5, bodies,
                                                              bodies.Length / 10, output), "ocean_body_buoyancy");
            return output;
        }

        // The hydrostatic pressure over the wetted triangles of a mesh shared by M bodies (ocean.h ocean_body_hydrostatics):
        // vertices [V][3] in the body frame, triangles [T][3] wound counter-clockwise seen from outside, bodies [M][10] as
        // Buoyancy takes them; per body 16 floats: sum F, wetted area, sum Tq about the origin, worst residual, the wetted
        // area's first moment, wet triangles, draught, wet vertices, sum Av.y, 0.  Force rho g out[0..2], torque
        // rho g out[4..6], heave stiffness rho g (-out[14]).  The reference has no counterpart.
        public float[] Hydrostatics(float[] vertices, int[] triangles, float[] bodies, int iterations = 4)
        {
            var output = new float[bodies.Length / 10 * OceanNative.HullRecordFloats];
            var pin = System.Runtime.InteropServices.GCHandle.Alloc(triangles, System.Runtime.InteropServices.GCHandleType.Pinned);
            try
            {
                OceanNative.Check(OceanNative.ocean_body_hydrostatics(ctx, 0, iterations, vertices, vertices.Length / 3,
                                                                      pin.AddrOfPinnedObject(), triangles.Length / 3, bodies,
                                                                      bodies.Length / 10, output), "ocean_body_hydrostatics");
            }
            finally
            {
                pin.Free();
            }
            return output;
        }

        // Buoyancy's records with the drag against the water's own velocity beside them (ocean.h ocean_body_dynamics;
        // `velocity` set before Awake): motion is [M][6] = (world linear velocity of the body origin, world angular
        // velocity); per body 16 floats: Buoyancy's 8, then sum F, sum T about the origin, the largest relative speed
        // over the wet probes and their number.  Drag force k out[8..10], torque k out[11..13] for the host's k; the
        // reference drags against still water (BuoyantObject.FixedUpdate: -rb.velocity * drag).
        public float[] Dynamics(float[] hull, float[] bodies, float[] motion, int iterations = 4,
                                int mode = OceanNative.QuerySurface, int law = OceanNative.DragLinear)
        {
            var output = new float[bodies.Length / 10 * 16];
            OceanNative.Check(OceanNative.ocean_body_dynamics(ctx, 0, mode, iterations, law, hull, hull.Length / 5, bodies,
                                                              motion, bodies.Length / 10, output), "ocean_body_dynamics");
            return output;
        }

        // BuoyantObject.FixedUpdate for M bodies of P probes each, `substeps` fixed updates against this frame's water in
        // one launch (ocean.h ocean_body_step; `velocity` set before Awake): state is [M][32] = (bodies' 10, motion's 6,
        // 16 ignored), props [M][4] = (1 / mass, 1 / Ix, 1 / Iy, 1 / Iz), step [8] = (h, g, B, kd, kt, la, aa, 0).  Per
        // body 32 floats: the state after the last substep, then Dynamics' record of that substep; the result is the
        // next call's state.
        public float[] StepBodies(float[] hull, float[] state, float[] props, float[] step, int substeps = 1,
                                  int iterations = 4, int mode = OceanNative.QuerySurface, int law = OceanNative.DragLinear)
        {
            var output = new float[state.Length];
            OceanNative.Check(OceanNative.ocean_body_step(ctx, 0, mode, iterations, law, substeps, step, hull, hull.Length / 5,
                                                          props, state, state.Length / 32, output), "ocean_body_step");
            return output;
        }

        // The velocity (x, y, z) of the water particle on the surface above (worldX, worldZ), at the last step's time
        // (ocean.h ocean_query_velocity; `velocity` set before Awake): what drag relative to the water and particle
        // advection need.  The reference has no counterpart: BuoyantObject drags against still water.
        public float[] GetWaterVelocity(float worldX, float worldZ, int iterations = 4)
        {
            var output = new float[8];
            OceanNative.Check(OceanNative.ocean_query_velocity(ctx, 0, iterations, new[] { worldX, worldZ }, 1, output),
                              "ocean_query_velocity");
            return new[] { output[0], output[1], output[2] };
        }

        // Physics.Raycast for the water (ocean.h ocean_raycast): the ray from `origin` along `direction` (the caller
        // keeps it unit) searched over [0, maxDistance] in `steps` intervals, then `refine` bisections.  False when
        // the ray stays above the water; else hit = 8 floats: distance, the ray point's height over the water there,
        // residual, status (OceanNative.RayHit, or RaySubmerged when the origin is under water), normal x, y, z,
        // foam.  The point met is origin + hit[0] * direction.  The reference has no counterpart.
        public bool Raycast(float[] origin, float[] direction, float maxDistance, out float[] hit, int iterations = 4,
                            int steps = 64, int refine = 8)
        {
            var ray = new[] { origin[0], origin[1], origin[2], direction[0], direction[1], direction[2], 0f, maxDistance };
            hit = new float[8];
            OceanNative.Check(OceanNative.ocean_raycast(ctx, 0, iterations, steps, refine, ray, 1, hit), "ocean_raycast");
            return (int)hit[3] != OceanNative.RayMiss;
        }

        // Where the sea is breaking (ocean.h ocean_whitecaps): the nodes (i, j) at (x0 + i dx, z0 + j dz) whose foam
        // reaches `threshold`, in ascending j * nx + i.  Returns T, the number of selected nodes; records = 8 floats
        // for each of the first min(T, capacity): displaced x, y, z, foam, the water's velocity x, y, z (`velocity`
        // set before Awake, else 0), (float)(j * nx + i).  Spawn points for spray and foam particles; the reference
        // has the foam only as a shading term (Water.shader:343).
        public int Whitecaps(float threshold, float x0, float z0, float dx, float dz, int nx, int ny, int capacity,
                             out float[] records, float lod = 0f)
        {
            // (a capacity outside the limits is refused by the library; no managed buffer of that size first)
            bool valid = capacity >= 1 && capacity <= OceanNative.WhitecapMaxRecords;
            var output = new float[((valid ? capacity : 0) + 1) * 8];
            OceanNative.Check(OceanNative.ocean_whitecaps(ctx, 0, lod, threshold, x0, z0, dx, dz, nx, ny, capacity, output,
                                                          (UIntPtr)(ulong)(output.Length * 4)), "ocean_whitecaps");
            int total = BitConverter.ToInt32(BitConverter.GetBytes(output[0]), 0);
            int written = BitConverter.ToInt32(BitConverter.GetBytes(output[1]), 0);
            records = new float[written * 8];
            Array.Copy(output, 8, records, 0, records.Length);
            return total;
        }

        // Spray particles (ocean.h ocean_spray_step): `pool` = (capacity + 1) * 8 floats, the header and the particles (8
        // floats each: position, age, velocity, tag); one fresh particle is spawned per record of the whitecap list
        // `emitters` ((emitCapacity + 1) * 8 floats as ocean_whitecaps writes it, or null); all take `substeps` substeps
        // under the 16 floats of `spray` against this frame's water, and those that fall back into the sea or outlive
        // their life are retired.  Returns the stepped pool, which is the next call's `pool`.  The reference has no
        // particles.
        public float[] Spray(float[] spray, float[] pool, float[] emitters = null, int substeps = 1, int iterations = 2)
        {
            int capacity = pool.Length / 8 - 1;
            int emitCapacity = emitters == null ? 0 : emitters.Length / 8 - 1;
            var output = new float[pool.Length];
            OceanNative.Check(OceanNative.ocean_spray_step(ctx, 0, iterations, substeps, spray, pool, capacity, emitters,
                                                           emitCapacity, output, (UIntPtr)(ulong)(output.Length * 4)),
                              "ocean_spray_step");
            return output;
        }

        // What a camera sees of the water (ocean.h ocean_camera): `camera` = 14 floats (eye, the direction through pixel
        // (0, 0), its change per column and per row, t0, t1).  OceanNative.CameraColor shades the fragment stage of
        // Water.shader with the 32 floats of `material` and returns r, g, b, status per pixel; CameraRange returns
        // the distance along each ray (+infinity where it misses), CameraHits Raycast's 8 floats per pixel; both take
        // a null material.  The headless stand-in for the reference's renderer.
        public float[] Camera(float[] camera, int width, int height, int mode = OceanNative.CameraColor,
                              float[] material = null, int iterations = 4, int steps = 64, int refine = 8)
        {
            int per = mode == OceanNative.CameraHits ? 8 : mode == OceanNative.CameraRange ? 1 : 4;
            // (a size outside the limits is refused by the library; no managed buffer of that size first)
            bool valid = width >= 1 && height >= 1 && (long)width * height <= OceanNative.CameraMaxPixels;
            var output = new float[valid ? width * height * per : 0];
            OceanNative.Check(OceanNative.ocean_camera(ctx, 0, mode, iterations, steps, refine, camera, material, width, height,
                                                       output, (UIntPtr)(ulong)(output.Length * 4)), "ocean_camera");
            return output;
        }

        // Camera with the boxes of `bodies` in the picture (ocean.h ocean_camera_bodies): `bodies` holds records `stride`
        // floats apart whose first ten floats are (c, q, s), the `bodies` of Buoyancy or the records StepBodies returns
        // (stride 32); `box` = (lo, hi) of the one box they share, `paint` = (r, g, b, ka), null outside the colour modes.
        // A body pixel has the status OceanNative.RayBody: its distance, its normal and the body's index in CameraHits.
        public float[] CameraBodies(float[] camera, int width, int height, float[] box, float[] paint, float[] bodies,
                                    int stride = 10, int mode = OceanNative.CameraColor, float[] material = null,
                                    int iterations = 4, int steps = 64, int refine = 8)
        {
            int per = mode == OceanNative.CameraHits ? 8 : mode == OceanNative.CameraRange ? 1 : 4;
            bool valid = width >= 1 && height >= 1 && (long)width * height <= OceanNative.CameraMaxPixels;
            var output = new float[valid ? width * height * per : 0];
            int count = bodies == null || stride < 10 ? 0 : (bodies.Length + stride - 10) / stride;
            OceanNative.Check(OceanNative.ocean_camera_bodies(ctx, 0, mode, iterations, steps, refine, camera, material, width,
                                                              height, box, paint, bodies, stride, count, output,
                                                              (UIntPtr)(ulong)(output.Length * 4)), "ocean_camera_bodies");
            return output;
        }

        // CameraBodies with the water seeing the bodies (ocean.h ocean_camera_scene): their shadows on it, their reflections
        // in it and their submerged parts through it.  `optics` = (shadow r, g, b, shadow intensity, water fog density, reach
        // of the secondary rays in metres); mode CameraColor, CameraColor | CameraSkyLut or CameraLinks (per pixel: lit or
        // not, the body seen through the water, the body reflected, the status).  Four floats per pixel in every mode.
        public float[] CameraScene(float[] camera, int width, int height, float[] box, float[] paint, float[] optics,
                                   float[] bodies, float[] material, int stride = 10, int mode = OceanNative.CameraColor,
                                   int iterations = 4, int steps = 64, int refine = 8)
        {
            bool valid = width >= 1 && height >= 1 && (long)width * height <= OceanNative.CameraMaxPixels;
            var output = new float[valid ? width * height * 4 : 0];
            int count = bodies == null || stride < 10 ? 0 : (bodies.Length + stride - 10) / stride;
            OceanNative.Check(OceanNative.ocean_camera_scene(ctx, 0, mode, iterations, steps, refine, camera, material, width,
                                                             height, box, paint, optics, bodies, stride, count, output,
                                                             (UIntPtr)(ulong)(output.Length * 4)), "ocean_camera_scene");
            return output;
        }

        // The atmosphere of AtmosphereController.cs (ocean.h "The atmosphere"): Awake's two tables, with `parameters` =
        // 32 floats (null: the reference's defaults) at the reference's sizes.
        public static readonly float[] DefaultAtmosphere = {
            6360000f, 6420000f, 5.802e-6f, 13.558e-6f, 6.5e-5f, 0f, 0f, 0f, 8000f, 3.996e-6f, 3.996e-6f, 3.996e-6f,
            4.4e-6f, 4.4e-6f, 4.4e-6f, 1200f, 0.85f, 0f, 0f, 0f, 0.65e-6f, 1.881e-6f, 0.085e-6f, 0f, 0f, 0f, 0.04f,
            0f, 0f, 0f, 0f, 0f };
        public void Atmosphere(float[] parameters = null)
        {
            OceanNative.Check(OceanNative.ocean_atmosphere(ctx, parameters ?? DefaultAtmosphere, 0, 0, 0, 0, 0, 0),
                              "ocean_atmosphere");
        }

        // AtmosphereController.Update: the sky-view table for the direction towards the sun, and the light's colour
        // (3 floats) for the camera's material.  Camera(..., OceanNative.CameraColor | OceanNative.CameraSkyLut) then
        // reflects that sky.
        public float[] SkyUpdate(float[] sun)
        {
            OceanNative.Check(OceanNative.ocean_sky_update(ctx, sun), "ocean_sky_update");
            var rgb = new float[3];
            OceanNative.Check(OceanNative.ocean_sun_color(ctx, sun, rgb), "ocean_sun_color");
            return rgb;
        }

        // One of the atmosphere's tables (OceanNative.LutTransmittance, LutMultiscatter, LutSkyView): 4 floats per texel.
        public float[] AtmosphereLut(int which, out int width, out int height)
        {
            IntPtr dev; UIntPtr w, h;
            OceanNative.Check(OceanNative.ocean_atmosphere_lut(ctx, which, out dev, out w, out h), "ocean_atmosphere_lut");
            width = (int)w; height = (int)h;
            var output = new float[width * height * 4];
            OceanNative.Check(OceanNative.ocean_atmosphere_read(ctx, which, output, (UIntPtr)(ulong)(output.Length * 4)),
                              "ocean_atmosphere_read");
            return output;
        }

        // The per-cascade bounds of the displacement (ocean.h ocean_surface_bounds): 8 floats per cascade, (min x, y,
        // z, w, max x, y, z, w); their cascade sums bound the displaced mesh (culling, tessellation range).
        public float[] SurfaceBounds()
        {
            var output = new float[cascades.Length * 8];
            OceanNative.Check(OceanNative.ocean_surface_bounds(ctx, 0, output, (UIntPtr)(ulong)(output.Length * 4)),
                              "ocean_surface_bounds");
            return output;
        }

        // Texture-out contract: device pointers for same-process renderers (WaterBody.cs:277-281).
        public IntPtr DeviceTexture(OceanTexture tex, out ulong bytes)
        {
            OceanNative.Check(OceanNative.ocean_get_device_ptr(ctx, tex, out var p, out var b), "ocean_get_device_ptr");
            bytes = (ulong)b;
            return p;
        }

        public void OnDisable() => Dispose();

        public void Dispose()
        {
            while (readbacks.Count > 0) OceanNative.ocean_readback_release(readbacks.Dequeue().req);
            foreach (var b in ring) OceanNative.ocean_host_free(b);
            ring.Clear();
            idle.Clear();
            if (ctx != IntPtr.Zero) OceanNative.ocean_destroy(ctx);
            ctx = IntPtr.Zero;
        }
    }
}
