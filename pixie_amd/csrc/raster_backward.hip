// pixie_amd/csrc/raster_backward.hip -- backward pass of the 3D Gaussian splatting rasteriser (raster.hip is the forward).
//
// One pixie_raster_backward call reads the workspace a pixie_raster_forward call left behind (centre, conic_opacity, offsets, ranges
// and the sorted instance list) and is the chain
//   hipMemsetAsync                    the per-instance buffer [instances][9]: slots of tiles the walk never reaches read as zero
//   raster_render_backward_kernel     one 256-thread workgroup per 16x16 tile
//   raster_gather_backward_kernel     one lane per Gaussian
// The render kernel stages 256 instances at a time in LDS like the forward and walks them FRONT TO BACK with the forward's own
// operations (raster_grad_math.h sample_backward), so T and the accumulated colour carry the forward's bits and nothing is recovered by
// division; what lies behind a sample is the pixel's final colour minus what has been accumulated.  It walks only up to the tile's
// largest n_contrib, and each lane ignores instances past its own.  Per staged Gaussian the nine partials are reduced over the tile in
// a fixed order: a butterfly over the wave (skipped when no lane of the wave contributes), then the four waves' partials through LDS,
// summed in wave order, and one lane writes the tile's nine floats to the per-instance buffer at slot offsets[g] + k, k being the
// tile's position in g's rectangle (raster_tile.h: instance_slot beside the duplicate kernels' emit_instances).  No floating-point atomics: gradients
// are bit-identical from run to run.  The gather kernel sums each Gaussian's contiguous segment sequentially and applies the
// per-Gaussian chain of raster_grad_math.h (projection, covariance, spherical harmonics).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "raster_grad_math.h"
#include "raster_math.h"
#include "raster_tile.h"
#include "raster_workspace.h"

using namespace pixie;
using namespace pixie::raster_tile;
using namespace pixie::raster_ws;
namespace rm = pixie::raster;

namespace {

constexpr int kWaves = kBlock / 64;
constexpr int kG = rm::kSampleGrads;

__global__ void __launch_bounds__(kBlock)
raster_render_backward_kernel(int W, int H, int tiles_x, int tiles_y, int n, uint64_t instances, const uint2* __restrict__ ranges, const uint32_t* __restrict__ point_list,
                              const float2* __restrict__ centre, const float4* __restrict__ conic_opacity, const float* __restrict__ colors,
                              const int32_t* __restrict__ radii, const uint64_t* __restrict__ offsets, const float* __restrict__ out_color,
                              const int32_t* __restrict__ n_contrib, const float* __restrict__ dL_dcolor, float* __restrict__ partials) {
    __shared__ float2 s_xy[kBlock];
    __shared__ float4 s_co[kBlock];
    __shared__ float3 s_rgb[kBlock];
    __shared__ uint64_t s_slot[kBlock];
    __shared__ float s_part[kWaves][kBlock][kG];     // 36 KiB
    __shared__ int s_max;
    const int tid = threadIdx.x;
    const int wave = tid >> 6, lane = tid & 63;
    const TilePixel px = tile_pixel(W, H);
    const uint2 range = tile_range(ranges, tiles_x, 0);

    rm::PixelGradWalk walk;
    walk.T = 1.0f; walk.r = walk.g = walk.b = 0.0f;
    walk.out_r = walk.out_g = walk.out_b = 0.0f;
    walk.gr = walk.gg = walk.gb = 0.0f;
    int last = 0;                                    // instances [0, last) of the tile's run are this pixel's to visit
    if (px.inside) {
        const size_t pix = (size_t)px.y * W + px.x;
        const size_t plane = (size_t)W * H;
        last = n_contrib[pix];
        walk.out_r = out_color[pix]; walk.out_g = out_color[plane + pix]; walk.out_b = out_color[2 * plane + pix];
        walk.gr = dL_dcolor[pix]; walk.gg = dL_dcolor[plane + pix]; walk.gb = dL_dcolor[2 * plane + pix];
    }
    const int run = range.y >= range.x && range.y <= instances ? (int)(range.y - range.x) : 0;
    if (last > run) last = run;                      // never past the tile's run, whatever n_contrib holds
    if (tid == 0) s_max = 0;
    __syncthreads();
    if (last > 0) atomicMax(&s_max, last);           // integer, in LDS
    __syncthreads();
    const int reach = s_max;                         // the tile's largest n_contrib: whole batches beyond it are skipped

    for (int start = 0; start < reach; start += kBlock) {
        const int cnt = reach - start < kBlock ? reach - start : kBlock;
        if (tid < cnt) {
            uint32_t g = point_list[range.x + (uint32_t)start + (uint32_t)tid];
            const bool sane = g < (uint32_t)n;       // a workspace that is not the forward's must not send a load or store astray
            if (!sane) g = 0u;
            const float2 c = stage_instance(tid, g, 0u, centre, conic_opacity, colors, s_xy, s_co, s_rgb);
            const uint64_t slot = instance_slot(c, radii[g], tiles_x, tiles_y, (int)blockIdx.x, (int)blockIdx.y, offsets[g]);
            s_slot[tid] = sane ? slot : instances;
        }
        __syncthreads();
        for (int j = 0; j < cnt; ++j) {              // block-uniform bounds: every lane takes part in every reduction
            float d[kG];
            for (int q = 0; q < kG; ++q) d[q] = 0.0f;
            bool hit = false;
            if (start + j < last) {
                const float2 xy = s_xy[j];
                const float4 co = s_co[j];
                const float3 rgb = s_rgb[j];
                hit = rm::sample_backward(walk, xy.x, xy.y, co.x, co.y, co.z, co.w, rgb.x, rgb.y, rgb.z, px.fx, px.fy, d);
            }
            if (__ballot(hit) != 0ull) {             // wave-uniform
                for (int q = 0; q < kG; ++q) {
                    float v = d[q];
                    for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
                    d[q] = v;
                }
            }
            if (lane == 0)
                for (int q = 0; q < kG; ++q) s_part[wave][j][q] = d[q];
        }
        __syncthreads();
        if (tid < cnt && s_slot[tid] < instances) {
            float* dst = partials + s_slot[tid] * kG;
            for (int q = 0; q < kG; ++q) {
                float v = s_part[0][tid][q];
                for (int w = 1; w < kWaves; ++w) v += s_part[w][tid][q];
                dst[q] = v;
            }
        }
        __syncthreads();                             // frees the staging buffers
    }
}

struct GatherArgs {
    const float* means;
    const float* cov3d;
    const float* scales;
    const float* rotations;
    const float* shs;
    const int32_t* radii;
    const uint64_t* offsets;
    const float* partials;
    float* d_means3d;
    float* d_means2d;
    float* d_opacity;
    float* d_colors;
    float* d_shs;
    float* d_cov3d;
    float* d_scales;
    float* d_rotations;
    uint64_t instances;
    float scale_modifier, campos[3];
    int n, sh_k, sh_degree;
};

__global__ void __launch_bounds__(kBlock)
raster_gather_backward_kernel(GatherArgs a, rm::Camera cam) {
    const int i = blockIdx.x * kBlock + threadIdx.x;
    if (i >= a.n) return;
    const size_t g = (size_t)i;
    float s[kG];
    for (int q = 0; q < kG; ++q) s[q] = 0.0f;
    const bool live = a.radii[i] > 0;
    if (live) {
        uint64_t end = a.offsets[g + 1];
        if (end > a.instances) end = a.instances;
        for (uint64_t k = a.offsets[g]; k < end; ++k) {
            const float* p = a.partials + k * kG;
            for (int q = 0; q < kG; ++q) s[q] += p[q];
        }
    }
    float dmean[3] = {0.0f, 0.0f, 0.0f}, dcov[6] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
    float ds[3] = {0.0f, 0.0f, 0.0f}, dq[4] = {0.0f, 0.0f, 0.0f, 0.0f};
    float p[3];
    for (int d = 0; d < 3; ++d) p[d] = a.means[g * 3 + d];
    if (a.shs) {
        float* dsh = a.d_shs ? a.d_shs + g * a.sh_k * 3 : nullptr;
        const int used = live ? (a.sh_degree + 1) * (a.sh_degree + 1) : 0;
        if (live) {
            const float vx = p[0] - a.campos[0], vy = p[1] - a.campos[1], vz = p[2] - a.campos[2];
            const float len = sqrtf(vx * vx + vy * vy + vz * vz);
            float ddir[3];
            rm::sh_backward(a.shs + g * a.sh_k * 3, a.sh_degree, vx / len, vy / len, vz / len, s + 6, dsh, ddir);
            rm::direction_backward(vx, vy, vz, ddir, dmean);
        }
        if (dsh)
            for (int k = used * 3; k < a.sh_k * 3; ++k) dsh[k] = 0.0f;
    }
    if (live) {
        float c6[6];
        if (a.cov3d) {
            for (int d = 0; d < 6; ++d) c6[d] = a.cov3d[g * 6 + d];
            rm::project_backward(p, c6, cam, s, s + 2, dcov, dmean);
        } else {
            float sc[3], q[4];
            for (int d = 0; d < 3; ++d) sc[d] = a.scales[g * 3 + d];
            for (int d = 0; d < 4; ++d) q[d] = a.rotations[g * 4 + d];
            rm::cov3d_from_scale_rot(sc, a.scale_modifier, q, c6);
            rm::project_backward(p, c6, cam, s, s + 2, dcov, dmean);
            rm::cov3d_backward(sc, a.scale_modifier, q, dcov, ds, dq);
        }
    }
    if (a.d_means3d)
        for (int d = 0; d < 3; ++d) a.d_means3d[g * 3 + d] = dmean[d];
    if (a.d_means2d) {
        a.d_means2d[g * 3] = s[0] * (0.5f * (float)cam.W);
        a.d_means2d[g * 3 + 1] = s[1] * (0.5f * (float)cam.H);
        a.d_means2d[g * 3 + 2] = 0.0f;
    }
    if (a.d_opacity) a.d_opacity[g] = s[5];
    if (a.d_colors)
        for (int d = 0; d < 3; ++d) a.d_colors[g * 3 + d] = s[6 + d];
    if (a.d_cov3d)
        for (int d = 0; d < 6; ++d) a.d_cov3d[g * 6 + d] = dcov[d];
    if (a.d_scales)
        for (int d = 0; d < 3; ++d) a.d_scales[g * 3 + d] = ds[d];
    if (a.d_rotations)
        for (int d = 0; d < 4; ++d) a.d_rotations[g * 4 + d] = dq[d];
}

size_t partial_bytes(int64_t instances) { return ((size_t)instances * kG * sizeof(float) + 255) & ~(size_t)255; }

}  // namespace

extern "C" {

int64_t pixie_raster_backward_workspace_bytes(int n, int width, int height, int64_t instances) {
    if (n < 0 || width <= 0 || height <= 0 || instances < 0 || instances > (int64_t)UINT32_MAX) {
        set_error("pixie_raster_backward_workspace_bytes: n %d, image %d x %d, instances %lld: n and instances must be >= 0, instances below 2^32, the image positive",
                  n, width, height, (long long)instances);
        return -1;
    }
    return (int64_t)partial_bytes(instances);
}

int pixie_raster_backward(const pixie_raster_backward_desc* d, void* stream) {
    const char* who = "pixie_raster_backward";
    PX_REQUIRE(d, "%s: null descriptor", who);
    const pixie_raster_desc& f = d->forward;
    const int n = f.n;
    if (check_forward_desc(who, "forward.", f)) return 1;
    PX_REQUIRE(d->instances >= 0 && d->instances <= (int64_t)UINT32_MAX, "%s: instances %lld outside [0, 2^32)", who, (long long)d->instances);
    PX_REQUIRE(f.d_final_T, "%s: null pointer (forward.d_final_T is required: render with it)", who);
    PX_REQUIRE(f.d_n_contrib, "%s: null pointer (forward.d_n_contrib is required: render with it)", who);
    PX_REQUIRE(d->d_dL_dcolor, "%s: null pointer (d_dL_dcolor is required)", who);
    PX_REQUIRE(!(d->d_dL_dcov3D && (d->d_dL_dscales || d->d_dL_drotations)),
               "%s: give d_dL_dcov3D or the pair d_dL_dscales, d_dL_drotations, as the forward took its covariance, not both", who);
    if (n > 0) {
        PX_REQUIRE(!d->d_dL_dcov3D || f.d_cov3d, "%s: d_dL_dcov3D given, but the forward took d_scales and d_rotations", who);
        PX_REQUIRE(!(d->d_dL_dscales || d->d_dL_drotations) || f.d_scales,
                   "%s: d_dL_dscales / d_dL_drotations given, but the forward took d_cov3d", who);
    }
    if (d->d_shs) {
        PX_REQUIRE(d->sh_degree >= 0 && d->sh_degree <= 3, "%s: sh_degree %d outside 0..3", who, d->sh_degree);
        PX_REQUIRE(d->sh_k >= (d->sh_degree + 1) * (d->sh_degree + 1), "%s: sh_k %d coefficients are fewer than sh_degree %d needs", who, d->sh_k,
                   d->sh_degree);
    } else {
        PX_REQUIRE(!d->d_dL_dshs, "%s: d_dL_dshs given without d_shs", who);
    }
    const size_t need = partial_bytes(d->instances);
    PX_REQUIRE(d->instances == 0 || (d->d_grad_workspace && d->grad_workspace_bytes >= (int64_t)need),
               "%s: d_grad_workspace of %lld bytes is smaller than the %lld bytes that %lld instances need", who,
               (long long)(d->d_grad_workspace ? d->grad_workspace_bytes : 0), (long long)need, (long long)d->instances);
    PX_REQUIRE(((uintptr_t)d->d_grad_workspace & 15) == 0, "%s: d_grad_workspace must be 16-byte aligned", who);
    const struct { float* p; size_t floats; } outs[] = {           // every gradient, with its floats per Gaussian
        {d->d_dL_dmeans3D, 3}, {d->d_dL_dmeans2D, 3}, {d->d_dL_dopacity, 1}, {d->d_dL_dcolors, 3}, {d->d_dL_dshs, 3 * (size_t)d->sh_k},
        {d->d_dL_dcov3D, 6}, {d->d_dL_dscales, 3}, {d->d_dL_drotations, 4}};
    bool asked = false;
    for (const auto& o : outs) asked = asked || o.p;
    if (!asked) return 0;                  // nothing asked for
    if (n == 0) return 0;                  // every output is empty
    const rm::Camera cam = rm::make_camera(f.viewmatrix, f.projmatrix, f.tanfovx, f.tanfovy, f.width, f.height);
    const int tiles = cam.tiles_x * cam.tiles_y;
    Layout L;
    if (make_layout(n, tiles, d->instances, L)) return 1;
    PX_REQUIRE(f.d_workspace && f.workspace_bytes >= (int64_t)L.total_bytes && ((uintptr_t)f.d_workspace & 15) == 0,
               "%s: forward.d_workspace of %lld bytes cannot be the 16-byte aligned workspace of a forward with %lld instances (%lld bytes)", who,
               (long long)f.workspace_bytes, (long long)d->instances, (long long)L.total_bytes);
    hipStream_t st = as_stream(stream);
    if (d->instances == 0) {
        for (const auto& o : outs)           // nothing was drawn: every gradient asked for is zero
            if (o.p) PX_CHECK_HIP(hipMemsetAsync(o.p, 0, sizeof(float) * o.floats * (size_t)n, st));
        return 0;
    }
    const char* ws = (const char*)f.d_workspace;
    const float2* centre = (const float2*)(ws + L.centre);
    const float4* conic_opacity = (const float4*)(ws + L.conic_opacity);
    const uint64_t* offsets = (const uint64_t*)(ws + L.offsets);
    const uint2* ranges = (const uint2*)(ws + L.ranges);
    const uint32_t* sorted_vals = (const uint32_t*)(ws + L.vals_out);
    float* partials = (float*)d->d_grad_workspace;
    PX_CHECK_HIP(hipMemsetAsync(partials, 0, (size_t)d->instances * kG * sizeof(float), st));
    hipLaunchKernelGGL(raster_render_backward_kernel, dim3(cam.tiles_x, cam.tiles_y), dim3(kBlock), 0, st, f.width, f.height, cam.tiles_x,
                       cam.tiles_y, n, (uint64_t)d->instances, ranges, sorted_vals, centre, conic_opacity, f.d_colors, (const int32_t*)f.d_radii, offsets,
                       (const float*)f.d_out_color, (const int32_t*)f.d_n_contrib, d->d_dL_dcolor, partials);
    PX_CHECK_HIP(hipGetLastError());
    GatherArgs a;
    a.means = f.d_means; a.cov3d = f.d_cov3d; a.scales = f.d_scales; a.rotations = f.d_rotations; a.shs = d->d_shs;
    a.radii = f.d_radii; a.offsets = offsets; a.partials = partials;
    a.d_means3d = d->d_dL_dmeans3D; a.d_means2d = d->d_dL_dmeans2D; a.d_opacity = d->d_dL_dopacity; a.d_colors = d->d_dL_dcolors;
    a.d_shs = d->d_dL_dshs; a.d_cov3d = d->d_dL_dcov3D; a.d_scales = d->d_dL_dscales; a.d_rotations = d->d_dL_drotations;
    a.instances = (uint64_t)d->instances;
    a.scale_modifier = f.scale_modifier;
    for (int k = 0; k < 3; ++k) a.campos[k] = d->campos[k];
    a.n = n; a.sh_k = d->sh_k; a.sh_degree = d->sh_degree;
    hipLaunchKernelGGL(raster_gather_backward_kernel, dim3(cdiv(n, kBlock)), dim3(kBlock), 0, st, a, cam);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
