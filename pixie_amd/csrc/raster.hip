// pixie_amd/csrc/raster.hip -- forward 3D Gaussian splatting rasteriser: the per-frame render of PG's frame loop
// (gs_simulation.py:610-619), and the device form of convert_SH (utils/render_utils.py:113-130).  Inference only.
//
// One pixie_raster_forward call is the chain
//   raster_preprocess_kernel   one lane per Gaussian: raster_math.h project() -> depth, centre, (conic, opacity), radius, tiles touched
//   hipcub ExclusiveSum        over n + 1 tile counts (the last is 0), so its last element is the instance count
//   [one stream synchronise: the host reads the instance count and checks that the workspace holds it]
//   raster_duplicate_kernel    per Gaussian, one (tile << 32 | depth bits, index) pair per tile of its rectangle
//   hipcub SortPairs           over 32 + ceil(log2(tiles)) bits; stable, so equal (tile, depth) keep index order
//   raster_ranges_kernel       one lane per instance: where each tile's run starts and ends
//   raster_render_kernel       one 256-thread workgroup per 16x16 tile
// The render kernel stages 256 instances at a time in LDS -- centre, conic + opacity and the colour (9 KiB) -- and every lane walks
// them front to back for its pixel.  Every LDS read in that walk has one address for the whole wave (a broadcast), so what bounds
// it is the wave's own instruction issue: per sample a ds_read_b64 and a ds_read_b128, ~28 VALU instructions up to the
// contribution branch (expf's range handling included) and, inside that branch, a ds_read_b96 for the colour.
//
// pixie_raster_forward_batch renders `views` frames of one Gaussian set with the same chain run once over views * n Gaussian-views
// (the raster_batch_* kernels): one projection launch, one scan, one synchronise that reads the views + 1 offsets at the view
// boundaries, then per group of consecutive views (raster_batch_plan.h) one duplicate / sort / ranges / render with the view in the
// key bits above the tile and in the render grid's z.  Same blend code, same order inside a (view, tile) run: same bits per image.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstdint>
#include <vector>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "raster_batch_plan.h"
#include "raster_math.h"
#include "raster_tile.h"
#include "raster_workspace.h"

using namespace pixie;
namespace rm = pixie::raster;
using namespace pixie::raster_tile;
using namespace pixie::raster_ws;

namespace {

__global__ void __launch_bounds__(kBlock)
raster_preprocess_kernel(int n, rm::Camera cam, const float* __restrict__ means, const float* __restrict__ cov3d, const float* __restrict__ scales,
                         const float* __restrict__ rotations, float scale_modifier, const float* __restrict__ opacity, float* __restrict__ depth,
                         float2* __restrict__ centre, float4* __restrict__ conic_opacity, int32_t* __restrict__ radii, uint64_t* __restrict__ tiles_touched) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    if (i == n) { tiles_touched[n] = 0; return; }    // the scan runs over n + 1 counts
    float p[3], c6[6];
    for (int d = 0; d < 3; ++d) p[d] = means[(size_t)i * 3 + d];
    if (cov3d) {
        for (int d = 0; d < 6; ++d) c6[d] = cov3d[(size_t)i * 6 + d];
    } else {
        float s[3], q[4];
        for (int d = 0; d < 3; ++d) s[d] = scales[(size_t)i * 3 + d];
        for (int d = 0; d < 4; ++d) q[d] = rotations[(size_t)i * 4 + d];
        rm::cov3d_from_scale_rot(s, scale_modifier, q, c6);
    }
    rm::Splat2D o;
    if (!rm::project(p, c6, cam, o)) { store_projection((size_t)i, i, nullptr, opacity, depth, centre, conic_opacity, radii, tiles_touched); return; }
    store_projection((size_t)i, i, &o, opacity, depth, centre, conic_opacity, radii, tiles_touched);
}

__global__ void __launch_bounds__(kBlock)
raster_duplicate_kernel(int n, int tiles_x, int tiles_y, const float2* __restrict__ centre, const float* __restrict__ depth, const int32_t* __restrict__ radii,
                        const uint64_t* __restrict__ offsets, uint64_t* __restrict__ keys, uint32_t* __restrict__ values) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int r = radii[i];
    if (r <= 0) return;
    emit_instances(centre[i], r, (uint64_t)__float_as_uint(depth[i]), tiles_x, tiles_y, 0u, (uint32_t)i, offsets[i], offsets[i + 1], keys, values);
}

__global__ void __launch_bounds__(kBlock)
raster_ranges_kernel(int64_t count, const uint64_t* __restrict__ keys, uint2* __restrict__ ranges) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= count) return;
    const uint32_t tile = (uint32_t)(keys[i] >> 32);
    if (i == 0) {
        ranges[tile].x = 0u;
    } else {
        const uint32_t prev = (uint32_t)(keys[i - 1] >> 32);
        if (prev != tile) {
            ranges[prev].y = (uint32_t)i;
            ranges[tile].x = (uint32_t)i;
        }
    }
    if (i == count - 1) ranges[tile].y = (uint32_t)count;
}

__global__ void __launch_bounds__(kBlock)
raster_render_kernel(int W, int H, int tiles_x, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list, const float2* __restrict__ centre,
                     const float4* __restrict__ conic_opacity, const float* __restrict__ colors, float bg0, float bg1, float bg2,
                     float* __restrict__ out_color, float* __restrict__ final_T, int32_t* __restrict__ n_contrib) {
    __shared__ float2 s_xy[kBlock];
    __shared__ float4 s_co[kBlock];
    __shared__ float3 s_rgb[kBlock];
    const TilePixel px = tile_pixel(W, H);
    const rm::PixelAcc acc = forward_walk(tile_range(ranges, tiles_x, 0), px, point_list, centre, conic_opacity, colors, 0u, s_xy, s_co, s_rgb);
    if (px.inside) {
        const size_t pix = (size_t)px.y * W + px.x;
        const size_t plane = (size_t)W * H;
        const float3 c = composite(acc, bg0, bg1, bg2);
        out_color[pix] = c.x;
        out_color[plane + pix] = c.y;
        out_color[2 * plane + pix] = c.z;
        if (final_T) final_T[pix] = acc.T;
        if (n_contrib) n_contrib[pix] = (int32_t)acc.last;
    }
}

__global__ void __launch_bounds__(kBlock)
sh_to_rgb_kernel(const float* __restrict__ shs, int64_t n, int k_coeffs, int degree, const float* __restrict__ pos, float cx, float cy,
                 float cz, const float* __restrict__ rot, int64_t n_rot, float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const float campos[3] = {cx, cy, cz};
    sh_colour(shs + i * k_coeffs * 3, degree, pos + i * 3, campos, i < n_rot ? rot + i * 9 : nullptr, out + i * 3);
}

// ------------------------------------------------------------------------------------------------ a batch of views
// Index conventions: a Gaussian-view is G = view * n + i over the whole batch (what preprocess and the scan see) and g = view in
// group * n + i inside a sort group (the sorted value).  i < n_dyn is a dynamic Gaussian, the rest is the static tail.
struct ViewCam {
    rm::Camera cam;
    float campos[3];
    float pad_;
};

struct BatchGeom {
    const float* means;                    // [views][n_dyn][3], view stride in elements
    const float* cov3d;
    int64_t means_stride, cov3d_stride;
    const float* static_means;             // [n - n_dyn][3]
    const float* static_cov3d;
    int n, n_dyn;
};

// raster_preprocess_kernel over (Gaussian, view): blockIdx.y is the view, so the camera is wave-uniform.  With shs it also evaluates
// the colour of every Gaussian that survives the projection, as sh_to_rgb_kernel does without a rotation.
__global__ void __launch_bounds__(kBlock)
raster_batch_preprocess_kernel(BatchGeom geo, int views, const ViewCam* __restrict__ cams, const float* __restrict__ opacity,
                               const float* __restrict__ shs, int k_coeffs, int sh_degree, float* __restrict__ depth, float2* __restrict__ centre,
                               float4* __restrict__ conic_opacity, int32_t* __restrict__ radii, float* __restrict__ rgb, uint64_t* __restrict__ tiles_touched) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    const int v = blockIdx.y;
    const int n = geo.n;
    if (i > n) return;
    if (i == n) {                                    // the scan runs over views * n + 1 counts
        if (v == views - 1) tiles_touched[(size_t)views * n] = 0;
        return;
    }
    const size_t G = (size_t)v * n + i;
    const float* mp = i < geo.n_dyn ? geo.means + (size_t)v * geo.means_stride + (size_t)i * 3 : geo.static_means + (size_t)(i - geo.n_dyn) * 3;
    const float* cp = i < geo.n_dyn ? geo.cov3d + (size_t)v * geo.cov3d_stride + (size_t)i * 6 : geo.static_cov3d + (size_t)(i - geo.n_dyn) * 6;
    float p[3], c6[6];
    for (int d = 0; d < 3; ++d) p[d] = mp[d];
    for (int d = 0; d < 6; ++d) c6[d] = cp[d];
    const ViewCam& vc = cams[v];
    rm::Splat2D o;
    if (!rm::project(p, c6, vc.cam, o)) { store_projection(G, i, nullptr, opacity, depth, centre, conic_opacity, radii, tiles_touched); return; }
    store_projection(G, i, &o, opacity, depth, centre, conic_opacity, radii, tiles_touched);
    if (shs)
        sh_colour(shs + (size_t)i * k_coeffs * 3, sh_degree, p, vc.campos, nullptr, rgb + G * 3);
}

// bounds[v] = offsets[v * n], v = 0 .. views: the instance offsets at the view boundaries, the only thing the host reads back
__global__ void __launch_bounds__(kBlock)
raster_batch_bounds_kernel(int views, int n, const uint64_t* __restrict__ offsets, uint64_t* __restrict__ bounds) {
    const int v = blockIdx.x * kBlock + threadIdx.x;
    if (v <= views) bounds[v] = offsets[(size_t)v * n];
}

// raster_duplicate_kernel for the views [v0, v0 + gridDim.y) of one group: keys carry (view in group * tiles + tile), values g
__global__ void __launch_bounds__(kBlock)
raster_batch_duplicate_kernel(int n, int v0, int tiles_x, int tiles_y, uint64_t group_base, uint64_t group_count,
                              const float2* __restrict__ centre, const float* __restrict__ depth, const int32_t* __restrict__ radii,
                              const uint64_t* __restrict__ offsets, uint64_t* __restrict__ keys, uint32_t* __restrict__ values) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int vg = blockIdx.y;
    const size_t G = (size_t)(v0 + vg) * n + i;
    const int r = radii[G];
    if (r <= 0) return;
    uint64_t end = offsets[G + 1] - group_base;
    if (end > group_count) end = group_count;        // never past what the host sized the group's buffers for
    emit_instances(centre[G], r, (uint64_t)__float_as_uint(depth[G]), tiles_x, tiles_y, (uint32_t)vg * (uint32_t)(tiles_x * tiles_y),
                   (uint32_t)((size_t)vg * n + i), offsets[G] - group_base, end, keys, values);
}

// raster_render_kernel on a (tiles_x, tiles_y, views in group) grid: the same walk and the same compositing per view; the epilogue
// also writes the 8-bit frame where one is asked for.
__global__ void __launch_bounds__(kBlock)
raster_batch_render_kernel(int W, int H, int tiles_x, int tiles_y, int n, int v0, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                           const float2* __restrict__ centre, const float4* __restrict__ conic_opacity, const float* __restrict__ colors,
                           int64_t colors_stride, float bg0, float bg1, float bg2, float* __restrict__ out_color, uint8_t* __restrict__ out_rgb8,
                           float* __restrict__ final_T, int32_t* __restrict__ n_contrib) {
    __shared__ float2 s_xy[kBlock];
    __shared__ float4 s_co[kBlock];
    __shared__ float3 s_rgb[kBlock];
    const int vg = blockIdx.z;
    const size_t view = (size_t)(v0 + vg);
    const size_t gbase = (size_t)v0 * n;                        // g -> G
    const TilePixel px = tile_pixel(W, H);
    const rm::PixelAcc acc = forward_walk(tile_range(ranges, tiles_x, (size_t)vg * (tiles_x * tiles_y)), px, point_list, centre + gbase,
                                          conic_opacity + gbase, colors + view * colors_stride, (uint32_t)((size_t)vg * n), s_xy, s_co, s_rgb);
    if (px.inside) {
        const size_t pix = (size_t)px.y * W + px.x;
        const size_t plane = (size_t)W * H;
        const float3 c = composite(acc, bg0, bg1, bg2);
        if (out_color) {
            float* oc = out_color + view * 3 * plane;
            oc[pix] = c.x;
            oc[plane + pix] = c.y;
            oc[2 * plane + pix] = c.z;
        }
        if (out_rgb8) {
            uint8_t* o8 = out_rgb8 + (view * plane + pix) * 3;
            o8[0] = (uint8_t)rintf(fminf(fmaxf(255.0f * c.x, 0.0f), 255.0f));
            o8[1] = (uint8_t)rintf(fminf(fmaxf(255.0f * c.y, 0.0f), 255.0f));
            o8[2] = (uint8_t)rintf(fminf(fmaxf(255.0f * c.z, 0.0f), 255.0f));
        }
        if (final_T) final_T[view * plane + pix] = acc.T;
        if (n_contrib) n_contrib[view * plane + pix] = (int32_t)acc.last;
    }
}

// Workspace of a batch: what the projection and the scan of views * n Gaussian-views need, then one group's sort storage.
struct BatchLayout : SortLayout {
    size_t cams, depth, centre, conic_opacity, radii, rgb, tiles_touched, offsets, bounds, ranges, scan_temp, scan_temp_bytes, fixed_bytes, total_bytes;
    int max_group_views;
};

constexpr int kSortProbes = 16;

int make_batch_layout(int n, int views, int tiles, int64_t instances, BatchLayout& L) {
    const size_t total = (size_t)views * (size_t)n;
    const int64_t by_key = (int64_t)UINT32_MAX / tiles;          // view in group * tiles + tile must fit 32 bits
    L.max_group_views = (int)(by_key < views ? by_key : views);
    size_t cur = 0;
    L.cams = take(cur, sizeof(ViewCam) * (size_t)views);
    L.depth = take(cur, sizeof(float) * total);
    L.centre = take(cur, sizeof(float2) * total);
    L.conic_opacity = take(cur, sizeof(float4) * total);
    L.radii = take(cur, sizeof(int32_t) * total);
    L.rgb = take(cur, sizeof(float) * 3 * total);
    L.tiles_touched = take(cur, sizeof(uint64_t) * (total + 1));
    L.offsets = take(cur, sizeof(uint64_t) * (total + 1));
    L.bounds = take(cur, sizeof(uint64_t) * ((size_t)views + 1));
    L.ranges = take(cur, sizeof(uint2) * (size_t)L.max_group_views * (size_t)tiles);
    L.scan_temp_bytes = 0;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_temp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (int)(total + 1)));
    L.scan_temp = take(cur, L.scan_temp_bytes);
    L.fixed_bytes = cur;
    const size_t m = (size_t)instances;
    // A group may hold any count up to m, and the library's storage need not grow monotonically with the count: take the largest
    // of a ladder of counts.  The call still checks each group's own need against what is left behind L.sort_temp.
    size_t temp = 0;
    for (int k = 1; k <= kSortProbes && m > 0; ++k) {
        size_t b = 0;
        if (sort_temp_bytes((m * k + kSortProbes - 1) / kSortProbes, (int64_t)L.max_group_views * tiles, b)) return 1;
        if (b > temp) temp = b;
    }
    take_sort(cur, m, temp, L);
    L.total_bytes = cur;
    return 0;
}

int check_batch_shape(const char* who, int n, int views, int width, int height, int64_t max_instances) {
    if (check_shape(who, n, width, height)) return 1;
    PX_REQUIRE(views >= 1 && views <= 65535, "%s: views %d outside 1..65535", who, views);
    PX_REQUIRE((int64_t)views * n < (int64_t)INT_MAX, "%s: views %d x n %d exceeds one scan (2^31 - 1 counts)", who, views, n);
    PX_REQUIRE(max_instances >= 0 && max_instances <= (int64_t)UINT32_MAX, "%s: max_instances %lld outside [0, 2^32)", who, (long long)max_instances);
    return 0;
}

// One sort group: sorts the `count` (key, value) pairs that a duplicate kernel left in S.keys_in / S.vals_in over `tiles` tiles (all
// the views of the group) and marks where each tile's run starts and ends in `ranges`, which the caller has zeroed.
int sort_group(char* ws, const SortLayout& S, uint64_t count, int64_t tiles, uint2* ranges, hipStream_t st) {
    size_t tb = 0;
    if (sort_temp_bytes((size_t)count, tiles, tb)) return 1;
    uint64_t* keys_out = (uint64_t*)(ws + S.keys_out);
    PX_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(ws + S.sort_temp, tb, (const uint64_t*)(ws + S.keys_in), keys_out, (const uint32_t*)(ws + S.vals_in),
                                                    (uint32_t*)(ws + S.vals_out), (size_t)count, 0, key_bits(tiles), st));
    hipLaunchKernelGGL(raster_ranges_kernel, dim3(cdiv((long)count, kBlock)), dim3(kBlock), 0, st, (int64_t)count, keys_out, ranges);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace

extern "C" {

int64_t pixie_raster_workspace_bytes(int n, int width, int height, int64_t max_instances) {
    if (check_batch_shape("pixie_raster_workspace_bytes", n, 1, width, height, max_instances)) return -1;      // one view
    const int tiles = cdiv(width, rm::kTile) * cdiv(height, rm::kTile);
    Layout L;
    if (make_layout(n, tiles, max_instances, L)) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_raster_forward(const pixie_raster_desc* d, int64_t* instances_out, void* stream) {
    PX_REQUIRE(d, "pixie_raster_forward: null descriptor");
    if (instances_out) *instances_out = 0;
    if (check_forward_desc("pixie_raster_forward", "", *d)) return 1;
    const int n = d->n;
    const rm::Camera cam = rm::make_camera(d->viewmatrix, d->projmatrix, d->tanfovx, d->tanfovy, d->width, d->height);
    const int tiles = cam.tiles_x * cam.tiles_y;
    Layout L;
    if (make_layout(n, tiles, 0, L)) return 1;
    PX_REQUIRE(d->d_workspace && d->workspace_bytes >= (int64_t)L.fixed_bytes,
               "pixie_raster_forward: workspace of %lld bytes is smaller than the %lld bytes that %d Gaussians and %d tiles need before any instance",
               (long long)d->workspace_bytes, (long long)L.fixed_bytes, n, tiles);
    PX_REQUIRE(((uintptr_t)d->d_workspace & 15) == 0, "pixie_raster_forward: d_workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    char* ws = (char*)d->d_workspace;
    float* depth = (float*)(ws + L.depth);
    float2* centre = (float2*)(ws + L.centre);
    float4* conic_opacity = (float4*)(ws + L.conic_opacity);
    uint64_t* tiles_touched = (uint64_t*)(ws + L.tiles_touched);
    uint64_t* offsets = (uint64_t*)(ws + L.offsets);
    uint2* ranges = (uint2*)(ws + L.ranges);

    uint64_t count = 0;
    if (n > 0) {
        hipLaunchKernelGGL(raster_preprocess_kernel, dim3(cdiv((long)n + 1, kBlock)), dim3(kBlock), 0, st, n, cam, d->d_means, d->d_cov3d,
                           d->d_scales, d->d_rotations, d->scale_modifier, d->d_opacity, depth, centre, conic_opacity, d->d_radii, tiles_touched);
        PX_CHECK_HIP(hipGetLastError());
        size_t tb = L.scan_temp_bytes;
        PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scan_temp, tb, (const uint64_t*)tiles_touched, offsets, n + 1, st));
        PX_CHECK_HIP(hipMemcpyAsync(&count, offsets + n, sizeof count, hipMemcpyDeviceToHost, st));
        PX_CHECK_HIP(hipStreamSynchronize(st));
    }
    if (instances_out) *instances_out = (int64_t)count;
    PX_REQUIRE(count <= (uint64_t)UINT32_MAX, "pixie_raster_forward: %llu instances exceed 2^32", (unsigned long long)count);
    if (make_layout(n, tiles, (int64_t)count, L)) return 1;
    PX_REQUIRE((int64_t)L.total_bytes <= d->workspace_bytes, "pixie_raster_forward: workspace too small: %llu instances need %lld bytes, the workspace has %lld",
               (unsigned long long)count, (long long)L.total_bytes, (long long)d->workspace_bytes);

    PX_CHECK_HIP(hipMemsetAsync(ranges, 0, sizeof(uint2) * (size_t)tiles, st));
    uint32_t* sorted_vals = (uint32_t*)(ws + L.vals_out);
    if (count > 0) {
        hipLaunchKernelGGL(raster_duplicate_kernel, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, st, n, cam.tiles_x, cam.tiles_y, centre, depth,
                           d->d_radii, offsets, (uint64_t*)(ws + L.keys_in), (uint32_t*)(ws + L.vals_in));
        PX_CHECK_HIP(hipGetLastError());
        if (sort_group(ws, L, count, tiles, ranges, st)) return 1;
    }
    hipLaunchKernelGGL(raster_render_kernel, dim3(cam.tiles_x, cam.tiles_y), dim3(kBlock), 0, st, d->width, d->height, cam.tiles_x, ranges, sorted_vals,
                       centre, conic_opacity, d->d_colors, d->bg[0], d->bg[1], d->bg[2], d->d_out_color, d->d_final_T, d->d_n_contrib);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_sh_to_rgb(const float* d_shs, int64_t n, int k_coeffs, int degree, const float* d_pos, const float campos[3], const float* d_rot,
                    int64_t n_rot, float* d_out, void* stream) {
    PX_REQUIRE(n >= 0, "pixie_sh_to_rgb: n %lld < 0", (long long)n);
    PX_REQUIRE(degree >= 0 && degree <= 3, "pixie_sh_to_rgb: degree %d outside 0..3", degree);
    PX_REQUIRE(k_coeffs >= (degree + 1) * (degree + 1), "pixie_sh_to_rgb: %d coefficients are fewer than degree %d needs", k_coeffs, degree);
    PX_REQUIRE(n_rot >= 0 && n_rot <= n, "pixie_sh_to_rgb: n_rot %lld outside [0, n]", (long long)n_rot);
    if (n == 0) return 0;
    PX_REQUIRE(d_shs && d_pos && campos && d_out, "pixie_sh_to_rgb: null pointer (d_shs, d_pos, campos and d_out are required)");
    PX_REQUIRE(n_rot == 0 || d_rot, "pixie_sh_to_rgb: n_rot %lld without d_rot", (long long)n_rot);
    PX_REQUIRE(n <= (int64_t)INT_MAX * kBlock / 2, "pixie_sh_to_rgb: n %lld exceeds one launch", (long long)n);
    hipLaunchKernelGGL(sh_to_rgb_kernel, dim3((unsigned)cdiv(n, kBlock)), dim3(kBlock), 0, as_stream(stream), d_shs, n, k_coeffs, degree, d_pos,
                       campos[0], campos[1], campos[2], d_rot, n_rot, d_out);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t pixie_raster_batch_workspace_bytes(int n, int views, int width, int height, int64_t max_instances) {
    if (check_batch_shape("pixie_raster_batch_workspace_bytes", n, views, width, height, max_instances)) return -1;
    const int tiles = cdiv(width, rm::kTile) * cdiv(height, rm::kTile);
    BatchLayout L;
    if (make_batch_layout(n, views, tiles, max_instances, L)) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_raster_forward_batch(const pixie_raster_batch_desc* d, int64_t* instances_out, int32_t* groups_out, void* stream) {
    const char* who = "pixie_raster_forward_batch";
    PX_REQUIRE(d, "%s: null descriptor", who);
    if (groups_out) *groups_out = 0;
    PX_REQUIRE(d->n_dyn >= 0 && d->n_static >= 0 && (int64_t)d->n_dyn + d->n_static < (int64_t)INT_MAX,
               "%s: n_dyn %d, n_static %d must be >= 0 and sum below 2^31 - 1", who, d->n_dyn, d->n_static);
    const int n = d->n_dyn + d->n_static, views = d->views;
    if (check_batch_shape(who, n, views, d->width, d->height, d->max_instances)) return 1;
    if (instances_out)
        for (int v = 0; v < views; ++v) instances_out[v] = 0;
    PX_REQUIRE(d->view, "%s: null pointer (view, the host array of per-view cameras, is required)", who);
    for (int v = 0; v < views; ++v)
        PX_REQUIRE(d->view[v].tanfovx > 0.0f && d->view[v].tanfovy > 0.0f, "%s: view %d: tanfovx %g, tanfovy %g must be positive", who, v,
                   d->view[v].tanfovx, d->view[v].tanfovy);
    PX_REQUIRE(d->d_out_color || d->d_out_rgb8, "%s: null pointer (one of d_out_color and d_out_rgb8 is required)", who);
    if (n > 0) {
        PX_REQUIRE(d->n_dyn == 0 || (d->d_means && d->d_cov3d), "%s: null pointer (d_means and d_cov3d are required for n_dyn %d)", who, d->n_dyn);
        PX_REQUIRE(d->n_static == 0 || (d->d_static_means && d->d_static_cov3d),
                   "%s: null pointer (d_static_means and d_static_cov3d are required for n_static %d)", who, d->n_static);
        PX_REQUIRE(d->means_view_stride >= 0 && d->cov3d_view_stride >= 0 && d->colors_view_stride >= 0, "%s: negative view stride", who);
        PX_REQUIRE(d->d_opacity, "%s: null pointer (d_opacity is required)", who);
        PX_REQUIRE((d->d_colors != nullptr) != (d->d_shs != nullptr), "%s: give exactly one of d_colors and d_shs", who);
        if (d->d_shs) {
            PX_REQUIRE(d->sh_degree >= 0 && d->sh_degree <= 3, "%s: sh_degree %d outside 0..3", who, d->sh_degree);
            PX_REQUIRE(d->k_coeffs >= (d->sh_degree + 1) * (d->sh_degree + 1), "%s: %d coefficients are fewer than degree %d needs", who,
                       d->k_coeffs, d->sh_degree);
        }
    }
    const int tiles_x = cdiv(d->width, rm::kTile), tiles_y = cdiv(d->height, rm::kTile), tiles = tiles_x * tiles_y;
    BatchLayout L;
    if (make_batch_layout(n, views, tiles, d->max_instances, L)) return 1;
    PX_REQUIRE(d->d_workspace && d->workspace_bytes >= (int64_t)L.total_bytes,
               "%s: workspace of %lld bytes is smaller than the %lld bytes that %d views of %d Gaussians, %d tiles and %lld instances need", who,
               (long long)d->workspace_bytes, (long long)L.total_bytes, views, n, tiles, (long long)d->max_instances);
    PX_REQUIRE(((uintptr_t)d->d_workspace & 15) == 0, "%s: d_workspace must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    char* ws = (char*)d->d_workspace;
    const ViewCam* cams = (const ViewCam*)(ws + L.cams);
    float* depth = (float*)(ws + L.depth);
    float2* centre = (float2*)(ws + L.centre);
    float4* conic_opacity = (float4*)(ws + L.conic_opacity);
    int32_t* radii = d->d_radii ? d->d_radii : (int32_t*)(ws + L.radii);
    float* rgb = (float*)(ws + L.rgb);
    uint64_t* tiles_touched = (uint64_t*)(ws + L.tiles_touched);
    uint64_t* offsets = (uint64_t*)(ws + L.offsets);
    uint64_t* d_bounds = (uint64_t*)(ws + L.bounds);
    uint2* ranges = (uint2*)(ws + L.ranges);

    std::vector<uint64_t> bounds((size_t)views + 1, 0), counts((size_t)views, 0);
    std::vector<ViewCam> host_cams;
    if (n > 0) {
        host_cams.resize((size_t)views);
        for (int v = 0; v < views; ++v) {
            const pixie_raster_view& pv = d->view[v];
            host_cams[v].cam = rm::make_camera(pv.viewmatrix, pv.projmatrix, pv.tanfovx, pv.tanfovy, d->width, d->height);
            for (int k = 0; k < 3; ++k) host_cams[v].campos[k] = pv.campos[k];
            host_cams[v].pad_ = 0.0f;
        }
        // host_cams and bounds outlive both copies: the synchronise below comes before either goes out of scope
        PX_CHECK_HIP(hipMemcpyAsync(ws + L.cams, host_cams.data(), sizeof(ViewCam) * (size_t)views, hipMemcpyHostToDevice, st));
        const BatchGeom geo = {d->d_means, d->d_cov3d, d->means_view_stride, d->cov3d_view_stride, d->d_static_means, d->d_static_cov3d, n, d->n_dyn};
        hipLaunchKernelGGL(raster_batch_preprocess_kernel, dim3(cdiv((long)n + 1, kBlock), views), dim3(kBlock), 0, st, geo, views, cams,
                           d->d_opacity, d->d_shs, d->k_coeffs, d->sh_degree, depth, centre, conic_opacity, radii, rgb, tiles_touched);
        PX_CHECK_HIP(hipGetLastError());
        size_t tb = L.scan_temp_bytes;
        PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(ws + L.scan_temp, tb, (const uint64_t*)tiles_touched, offsets, (int)((size_t)views * n + 1), st));
        hipLaunchKernelGGL(raster_batch_bounds_kernel, dim3(cdiv((long)views + 1, kBlock)), dim3(kBlock), 0, st, views, n, offsets, d_bounds);
        PX_CHECK_HIP(hipGetLastError());
        PX_CHECK_HIP(hipMemcpyAsync(bounds.data(), d_bounds, sizeof(uint64_t) * ((size_t)views + 1), hipMemcpyDeviceToHost, st));
        PX_CHECK_HIP(hipStreamSynchronize(st));      // the only one of the call
    }
    for (int v = 0; v < views; ++v) {
        counts[v] = bounds[v + 1] - bounds[v];
        if (instances_out) instances_out[v] = (int64_t)counts[v];
    }
    std::vector<int32_t> begin((size_t)views + 1, 0);
    const int64_t groups = rm::plan_groups(counts.data(), views, (uint64_t)d->max_instances, L.max_group_views, begin.data());
    if (groups < 0) {
        const int v = (int)(-1 - groups);
        return set_error("%s: workspace too small: view %d alone has %llu instances, max_instances is %lld", who, v,
                         (unsigned long long)counts[v], (long long)d->max_instances);
    }
    // every group's sort must find its temporary storage behind L.sort_temp before anything is rendered
    const size_t temp_room = (size_t)d->workspace_bytes - L.sort_temp;
    for (int64_t k = 0; k < groups; ++k) {
        const uint64_t count = bounds[begin[k + 1]] - bounds[begin[k]];
        size_t need = 0;
        if (sort_temp_bytes((size_t)count, (int64_t)(begin[k + 1] - begin[k]) * tiles, need)) return 1;
        PX_REQUIRE(need <= temp_room, "%s: workspace too small: sorting the %llu instances of views %d..%d needs %llu bytes of temporary storage, %llu are left",
                   who, (unsigned long long)count, begin[k], begin[k + 1] - 1, (unsigned long long)need, (unsigned long long)temp_room);
    }
    if (groups_out) *groups_out = (int32_t)groups;

    uint32_t* sorted_vals = (uint32_t*)(ws + L.vals_out);
    const float* colors = d->d_shs ? rgb : d->d_colors;
    const int64_t colors_stride = d->d_shs ? (int64_t)n * 3 : d->colors_view_stride;
    for (int64_t k = 0; k < groups; ++k) {
        const int v0 = begin[k], gv = begin[k + 1] - begin[k];
        const uint64_t count = bounds[v0 + gv] - bounds[v0];
        const int64_t group_tiles = (int64_t)gv * tiles;
        PX_CHECK_HIP(hipMemsetAsync(ranges, 0, sizeof(uint2) * (size_t)group_tiles, st));
        if (count > 0) {
            hipLaunchKernelGGL(raster_batch_duplicate_kernel, dim3(cdiv(n, kBlock), gv), dim3(kBlock), 0, st, n, v0, tiles_x, tiles_y, bounds[v0],
                               count, centre, depth, radii, offsets, (uint64_t*)(ws + L.keys_in), (uint32_t*)(ws + L.vals_in));
            PX_CHECK_HIP(hipGetLastError());
            if (sort_group(ws, L, count, group_tiles, ranges, st)) return 1;
        }
        hipLaunchKernelGGL(raster_batch_render_kernel, dim3(tiles_x, tiles_y, gv), dim3(kBlock), 0, st, d->width, d->height, tiles_x, tiles_y, n,
                           v0, ranges, sorted_vals, centre, conic_opacity, colors, colors_stride, d->bg[0], d->bg[1], d->bg[2], d->d_out_color,
                           d->d_out_rgb8, d->d_final_T, d->d_n_contrib);
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
