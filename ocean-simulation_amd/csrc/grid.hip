// Surface grids (ocean_surface_grid*): the surface over the nodes of a regular grid, for the two
// consumers that read it over an area and not at scattered points.
//
// The reference's renderer builds a regular plane (MeshGenerator.cs:19-35: planeSize / trianglesSize
// cells a side, 101 x 101 vertices by default) and the domain stage of Water.shader (:314-334) moves
// every vertex by the cascade-summed displacement at its world position; a heightfield collider or
// a top-down map wants the height above every node.  A grid is six numbers, (x0, z0, dx, dz, nx, ny):
// node (i, j), i < nx along world x and j < ny along world z, lies at
//     qx = x0 + (float)i * dx,  qz = z0 + (float)j * dz      (one fp32 multiply, one fp32 add each)
// and its result is element j * nx + i of the output.  Three modes, each defined by an entry that
// already exists (S = sample_cascades of sample_filter.h, the same operations in the same order):
//
//   OCEAN_GRID_VERTICES     k_sample_world at (qx, qz, lod): the displaced vertex
//                           (qx + S.disp.x, S.disp.y, qz + S.disp.z), the foam, the normal and a zero.
//   OCEAN_GRID_SURFACE      k_query_surface at (qx, qz) with K iterations: its 8-float record.
//   OCEAN_GRID_HEIGHTFIELD  element 0 of that record alone, float[ny][nx].
//
// No point list is read: the nodes follow from the six numbers, so a launch moves 8-12 B per node
// less than the point-list kernels.  What this kernel chooses is the mapping of nodes to lanes: one
// lane per node, a 256-thread workgroup covers a TW x (256 / TW) tile of nodes with x fastest, so a
// wave is TW x (64 / TW) nodes and the bilinear footprints of its lanes overlap along both axes.  TW =
// 64 is a strip of one row per wave, 32 and 16 are blocked; docs/MEASUREMENTS.md has all three.  The
// K loop is uniform over the launch, the edges of partial tiles are guarded per lane.
//
// No LDS, no atomics, no inline assembly: a gather of 4-16 texels per cascade and step through
// L1 / L2 / Infinity Cache, each step's taps depending on the one before (no roofline claimed).
#include "ocean_internal.h"
#include "sample_filter.h"
#include "spectrum_math.h"

namespace ocean {
namespace {

// Tiles are numbered x fastest over a 1-D launch (a grid of one column may be 2^22 nodes tall, more
// tiles than a launch's y dimension takes).
template <int TW, int MODE>
__global__ __launch_bounds__(256) void k_surface_grid(DevView v, int tile, int iterations, float lod, float x0,
                                                      float z0, float dx, float dz, int nx, int ny,
                                                      unsigned tiles_x, float* __restrict__ out) {
    constexpr int TH = 256 / TW;
    const unsigned by = blockIdx.x / tiles_x, bx = blockIdx.x - by * tiles_x;
    const int i = (int)(bx * TW + threadIdx.x % TW), j = (int)(by * TH + threadIdx.x / TW);
    if (i >= nx || j >= ny) return;
    const float2 q = grid_node(i, j, x0, z0, dx, dz);
    const float qx = q.x, qz = q.y;
    const size_t k = (size_t)j * nx + i;
    if (MODE == OCEAN_GRID_VERTICES) {
        const WorldSample s = sample_cascades(v, tile, qx, qz, lod);
        float4* o = reinterpret_cast<float4*>(out) + 2 * k;
        o[0] = make_float4(qx + s.disp.x, s.disp.y, qz + s.disp.z, s.turb);  // Water.shader:326-327
        o[1] = normal_from_deriv(s.deriv.x, s.deriv.y, s.deriv.z, s.deriv.w);
        return;
    }
    const float2 p = surface_fixed_point(v, tile, qx, qz, iterations);
    if (MODE == OCEAN_GRID_HEIGHTFIELD) {
        out[k] = sample_disp(v, tile, p.x, p.y).y;  // bit-identical to sample_cascades(...).disp.y
        return;
    }
    const SurfaceRecord rec = surface_record(sample_cascades(v, tile, p.x, p.y, 0.0f), p, qx, qz);
    float4* o = reinterpret_cast<float4*>(out) + 2 * k;
    o[0] = rec.at;
    o[1] = rec.nf;
}

}  // namespace

bool grid_tile_supported(int tile_w) { return tile_w == 64 || tile_w == 32 || tile_w == 16; }

hipError_t launch_surface_grid(const DevView& v, int tile, int mode, int iterations, float lod, float x0, float z0,
                               float dx, float dz, int nx, int ny, int tile_w, float* out, hipStream_t s) {
    if (nx <= 0 || ny <= 0) return hipSuccess;
    if (mode < OCEAN_GRID_VERTICES || mode > OCEAN_GRID_HEIGHTFIELD || !grid_tile_supported(tile_w))
        return hipErrorInvalidValue;
    (void)with_constant<64, 32, 16>(tile_w, [&](auto tw) {  // both values were checked above: one of each matches
        (void)with_constant<OCEAN_GRID_VERTICES, OCEAN_GRID_SURFACE, OCEAN_GRID_HEIGHTFIELD>(mode, [&](auto m) {
            constexpr int TW = decltype(tw)::value, TH = 256 / TW;
            const unsigned tiles_x = (unsigned)((nx + TW - 1) / TW), tiles_y = (unsigned)((ny + TH - 1) / TH);
            // nx * ny <= OCEAN_GRID_MAX_NODES = 2^22: at most 2^22 / TH + tiles_y < 2^31 tiles
            launch(k_surface_grid<TW, decltype(m)::value>, dim3(tiles_x * tiles_y), dim3(256), 0, s, v, tile, iterations,
                   lod, x0, z0, dx, dz, nx, ny, tiles_x, out);
        });
    });
    return hipGetLastError();
}

}  // namespace ocean
