// pixie_amd/csrc/raster_tile.h -- the device code the rasteriser's kernels share (raster.hip: single view and batch; raster_backward.hip):
// one body for every operation that must give the same bits on every path, the kernels being thin entry points around them.  A
// single-view kernel passes literal zeros for the offsets only a batch has (tile0, g0), which the compiler folds away.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "raster_math.h"

namespace pixie {
namespace raster_tile {

namespace rm = pixie::raster;

constexpr int kBlock = 256;               // = kTile * kTile: one lane per pixel of a tile

// ------------------------------------------------------------------------------------------------ per Gaussian
// Stores what the projection of Gaussian-view G (Gaussian i of its view) gave -- depth, centre, (conic, opacity), radius and tile
// count -- or, where it cannot be projected (o null), radius and count 0.  The caller branches on rm::project's result and passes a
// literal null on that side: projecting inside this function costs the single-view kernel two VGPRs.
__device__ __forceinline__ void store_projection(size_t G, int i, const rm::Splat2D* o, const float* opacity, float* depth, float2* centre,
                                                 float4* conic_opacity, int32_t* radii, uint64_t* tiles_touched) {
    if (!o) {
        radii[G] = 0;
        tiles_touched[G] = 0;
        return;
    }
    depth[G] = o->depth;
    centre[G] = make_float2(o->px, o->py);
    conic_opacity[G] = make_float4(o->ca, o->cb, o->cc, opacity[i]);
    radii[G] = o->radius;
    tiles_touched[G] = (uint64_t)((o->x1 - o->x0) * (o->y1 - o->y0));
}

// out[0..2] = the colour of the SH coefficients shs_i seen from campos at p, the direction first rotated by R (3x3) where R is given
__device__ __forceinline__ void sh_colour(const float* shs_i, int degree, const float* p, const float* campos, const float* R, float* out) {
    float dx = p[0] - campos[0], dy = p[1] - campos[1], dz = p[2] - campos[2];
    if (R) {
        const float rx = R[0] * dx + R[1] * dy + R[2] * dz;
        const float ry = R[3] * dx + R[4] * dy + R[5] * dz;
        const float rz = R[6] * dx + R[7] * dy + R[8] * dz;
        dx = rx; dy = ry; dz = rz;
    }
    const float len = sqrtf(dx * dx + dy * dy + dz * dz);
    float rgb[3];
    rm::sh_to_rgb(shs_i, degree, dx / len, dy / len, dz / len, rgb);
    for (int d = 0; d < 3; ++d) out[d] = rgb[d];
}

// The instances of one Gaussian: a (tile0 + tile << 32 | depth bits, value) pair per tile of its rectangle, row by row, in
// [off, end).  instance_slot below is the inverse and must enumerate in this order.
__device__ __forceinline__ void emit_instances(float2 c, int radius, uint64_t dbits, int tiles_x, int tiles_y, uint32_t tile0, uint32_t value,
                                               uint64_t off, uint64_t end, uint64_t* keys, uint32_t* values) {
    int x0, y0, x1, y1;
    rm::tile_rect(c.x, c.y, radius, tiles_x, tiles_y, x0, y0, x1, y1);
    for (int y = y0; y < y1; ++y)
        for (int x = x0; x < x1; ++x) {
            if (off >= end) return;              // never written past: the rectangle is the one the projection counted
            keys[off] = ((uint64_t)(tile0 + (uint32_t)(y * tiles_x + x)) << 32) | dbits;
            values[off] = value;
            ++off;
        }
}

// where emit_instances put tile (tile_x, tile_y) of the Gaussian whose instances start at `offset`
__device__ __forceinline__ uint64_t instance_slot(float2 c, int radius, int tiles_x, int tiles_y, int tile_x, int tile_y, uint64_t offset) {
    int x0, y0, x1, y1;
    rm::tile_rect(c.x, c.y, radius, tiles_x, tiles_y, x0, y0, x1, y1);
    return offset + (uint64_t)((tile_y - y0) * (x1 - x0) + (tile_x - x0));
}

// ------------------------------------------------------------------------------------------------ per tile
struct TilePixel { int x, y; bool inside; float fx, fy; };      // inside: of the image

// this lane's pixel of tile (blockIdx.x, blockIdx.y): wave w owns rows 4w .. 4w+3 of the tile
__device__ __forceinline__ TilePixel tile_pixel(int W, int H) {
    TilePixel p;
    p.x = blockIdx.x * rm::kTile + (threadIdx.x & (rm::kTile - 1));
    p.y = blockIdx.y * rm::kTile + (threadIdx.x >> 4);
    p.inside = p.x < W && p.y < H;
    p.fx = (float)p.x, p.fy = (float)p.y;
    return p;
}

// the run of sorted instances of this workgroup's tile; tile0 = the first tile of its view within the sort group
__device__ __forceinline__ uint2 tile_range(const uint2* ranges, int tiles_x, size_t tile0) {
    return ranges[tile0 + (blockIdx.y * tiles_x + blockIdx.x)];
}

// Stages sorted value g in LDS slot `at`: centre and (conic, opacity) of Gaussian-view g, colour of Gaussian g - g0.  Returns the centre.
__device__ __forceinline__ float2 stage_instance(int at, uint32_t g, uint32_t g0, const float2* centre, const float4* conic_opacity,
                                                 const float* colors, float2* s_xy, float4* s_co, float3* s_rgb) {
    const float2 c = centre[g];
    s_xy[at] = c;
    s_co[at] = conic_opacity[g];
    const size_t ci = (size_t)(g - g0) * 3;
    s_rgb[at] = make_float3(colors[ci], colors[ci + 1], colors[ci + 2]);
    return c;
}

// The forward walk of one tile: stages kBlock instances of `range` at a time and blends them front to back into this lane's pixel.
// centre and conic_opacity are indexed by the sorted value g, colors by g - g0.
__device__ __forceinline__ rm::PixelAcc forward_walk(uint2 range, const TilePixel& px, const uint32_t* point_list, const float2* centre,
                                                     const float4* conic_opacity, const float* colors, uint32_t g0, float2* s_xy, float4* s_co,
                                                     float3* s_rgb) {
    const int tid = threadIdx.x;
    int todo = (int)(range.y - range.x);
    rm::PixelAcc acc = rm::pixel_start(!px.inside);
    for (uint32_t base = range.x; base < range.y; base += kBlock, todo -= kBlock) {
        if (__syncthreads_count(acc.done) == kBlock) break;      // also the barrier that frees the staging buffers
        if (base + tid < range.y) stage_instance(tid, point_list[base + tid], g0, centre, conic_opacity, colors, s_xy, s_co, s_rgb);
        __syncthreads();
        const int cnt = todo < kBlock ? todo : kBlock;
        for (int j = 0; !acc.done && j < cnt; ++j) {
            const float2 xy = s_xy[j];
            const float4 co = s_co[j];
            const float3 rgb = s_rgb[j];
            rm::blend(acc, xy.x, xy.y, co.x, co.y, co.z, co.w, rgb.x, rgb.y, rgb.z, px.fx, px.fy);
        }
    }
    return acc;
}

// the pixel's colour over the background
__device__ __forceinline__ float3 composite(const rm::PixelAcc& acc, float bg0, float bg1, float bg2) {
    return make_float3(acc.r + acc.T * bg0, acc.g + acc.T * bg1, acc.b + acc.T * bg2);
}

}  // namespace raster_tile
}  // namespace pixie
