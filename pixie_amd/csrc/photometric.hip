// pixie_amd/csrc/photometric.hip -- the photometric loss of 3DGS training, gaussian-splatting/utils/loss_utils.py: l1_loss and
// ssim (window 11, sigma 1.5, zero padding 5, one window per channel, C1 = 1e-4, C2 = 9e-4) in one pass over the two images, and
// their gradient with respect to the first image in one more.
//
//   photometric_forward_kernel<kGrad>   one 256-thread workgroup per 16 x 16 output tile of one (image, channel) plane.  The
//                        26 x 26 halo'd tiles of both images go to LDS, zeros outside the image (the reference's zero padding);
//                        the horizontal 11-tap pass over a, b, a a, b b, a b goes to LDS (26 rows x 16 columns x 5), the vertical
//                        pass runs in registers.  Each pixel forms mu1, mu2, sigma1^2, sigma2^2, sigma12 and its SSIM value;
//                        with kGrad it also stores the three planes d mu, d S1, d S12 the backward convolves (below).
//                        sum(ssim) and sum(|a - b|) are reduced over the workgroup in a fixed order (wave shuffles, then the four
//                        waves in turn) into the workgroup's own slot.
//   photometric_finalise_kernel   one workgroup per image: every thread adds a fixed stride of slots in double, a fixed tree in
//                        LDS adds the 256 partial sums, thread 0 writes the two means.
//   photometric_backward_kernel   the same tiling over the three stored planes: with map = A1 A2 / (B1 B2), A1 = 2 mu1 mu2 + C1,
//                        A2 = 2 sigma12 + C2, B1 = mu1^2 + mu2^2 + C1, B2 = sigma1^2 + sigma2^2 + C2,
//                            d S1  = -map / B2                      (d map / d conv(a a))
//                            d S12 = 2 A1 / (B1 B2)                 (d map / d conv(a b))
//                            d mu  = 2 mu2 A2 / (B1 B2) - 2 mu1 map / B1 - 2 mu1 d S1 - mu2 d S12      (d map / d conv(a), total)
//                            d sum(map) / d a(p) = conv(d mu)(p) + 2 a(p) conv(d S1)(p) + b(p) conv(d S12)(p)
//                        with the same zero-padded symmetric window, and one store per pixel:
//                            g_l1 sign(a - b) / N + g_ssim (that) / N,     sign(0) = 0,  N = C H W per image.
// The window is built as the reference builds it -- exp in double, rounded to float32, divided by the float32 sum -- and applied
// separably; the reference applies the 121-tap outer product, which differs at rounding level.  No floating-point atomics; no host
// synchronise; the scalars stay on the device.  Results are bit-identical from run to run.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"

using namespace pixie;

namespace {

constexpr int kTile = 16;
constexpr int kRadius = 5;
constexpr int kTaps = 2 * kRadius + 1;
constexpr int kHalo = kTile + 2 * kRadius;      // 26
constexpr int kBlock = kTile * kTile;           // 256
constexpr float kC1 = 0.01f * 0.01f, kC2 = 0.03f * 0.03f;

struct Window {
    float w[kTaps];
};

// The reference's window: exp in double rounded to float32, divided by the taps' float32 sum.  torch adds the eleven taps with
// several accumulators and arrives at the correctly rounded sum; adding them one after the other in float32 lands one ulp below,
// which shifts every weight and biases a mean SSIM by 4e-7.  So: the sum in double, rounded once.
Window make_window() {
    Window win;
    double sum = 0.0;
    for (int x = 0; x < kTaps; ++x) {
        win.w[x] = (float)std::exp(-(double)((x - kRadius) * (x - kRadius)) / (2.0 * 1.5 * 1.5));
        sum += (double)win.w[x];
    }
    const float fsum = (float)sum;
    for (int x = 0; x < kTaps; ++x) win.w[x] /= fsum;
    return win;
}

struct Layout {
    int tiles_x, tiles_y;
    int64_t slots;                        // workgroups = b * c * tiles_x * tiles_y; two floats each
    size_t planes, plane_floats, total_bytes;
};

int make_layout(int b, int c, int h, int w, int with_grad, Layout& L, const char* who) {
    PX_REQUIRE(b >= 1 && c >= 1 && h >= 1 && w >= 1, "%s: b %d, c %d, h %d, w %d must all be positive", who, b, c, h, w);
    PX_REQUIRE(h <= 32768 && w <= 32768, "%s: images of %d x %d exceed 32768 a side", who, h, w);
    PX_REQUIRE((int64_t)b * c <= 65535, "%s: b * c = %lld planes exceed 65535", who, (long long)b * c);
    L.tiles_x = (w + kTile - 1) / kTile;
    L.tiles_y = (h + kTile - 1) / kTile;
    L.slots = (int64_t)b * c * L.tiles_x * L.tiles_y;
    PX_REQUIRE((int64_t)b * c * h * w < ((int64_t)1 << 40), "%s: %lld pixels exceed 2^40", who, (long long)b * c * h * w);
    L.plane_floats = (size_t)b * c * h * w;
    L.planes = (sizeof(float) * 2 * (size_t)L.slots + 255) & ~(size_t)255;
    L.total_bytes = L.planes + (with_grad ? 3 * sizeof(float) * L.plane_floats : 0);
    return 0;
}

// fixed-order sum over the workgroup; the result is valid in thread 0
__device__ __forceinline__ float block_sum(float v, float* s_red) {
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s, 64);
    const int wave = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) s_red[wave] = v;
    __syncthreads();
    return ((s_red[0] + s_red[1]) + s_red[2]) + s_red[3];
}

template <bool kGrad>
__global__ void __launch_bounds__(kBlock)
photometric_forward_kernel(const float* __restrict__ img, const float* __restrict__ gt, int h, int w, int tiles_x, Window win,
                           float* __restrict__ slots, float* __restrict__ planes, size_t plane_floats) {
    __shared__ float s_a[kHalo][kHalo], s_b[kHalo][kHalo];
    __shared__ float s_h[5][kHalo][kTile];
    __shared__ float s_red[2][kBlock / 64];
    const int tid = threadIdx.x;
    const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
    const size_t plane = (size_t)blockIdx.y * h * w;
    const int x0 = tile_x * kTile - kRadius, y0 = tile_y * kTile - kRadius;

    for (int k = tid; k < kHalo * kHalo; k += kBlock) {
        const int r = k / kHalo, c = k - r * kHalo;
        const int y = y0 + r, x = x0 + c;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        s_a[r][c] = in ? img[plane + (size_t)y * w + x] : 0.0f;
        s_b[r][c] = in ? gt[plane + (size_t)y * w + x] : 0.0f;
    }
    __syncthreads();
    for (int k = tid; k < kHalo * kTile; k += kBlock) {
        const int r = k / kTile, c = k - r * kTile;
        float sa = 0.0f, sb = 0.0f, saa = 0.0f, sbb = 0.0f, sab = 0.0f;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            const float a = s_a[r][c + t], b = s_b[r][c + t], wt = win.w[t];
            sa += wt * a; sb += wt * b; saa += wt * (a * a); sbb += wt * (b * b); sab += wt * (a * b);
        }
        s_h[0][r][c] = sa; s_h[1][r][c] = sb; s_h[2][r][c] = saa; s_h[3][r][c] = sbb; s_h[4][r][c] = sab;
    }
    __syncthreads();

    const int tx = tid % kTile, ty = tid / kTile;
    const int x = tile_x * kTile + tx, y = tile_y * kTile + ty;
    float mu1 = 0.0f, mu2 = 0.0f, eaa = 0.0f, ebb = 0.0f, eab = 0.0f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const float wt = win.w[t];
        mu1 += wt * s_h[0][ty + t][tx]; mu2 += wt * s_h[1][ty + t][tx];
        eaa += wt * s_h[2][ty + t][tx]; ebb += wt * s_h[3][ty + t][tx]; eab += wt * s_h[4][ty + t][tx];
    }
    float v_ssim = 0.0f, v_l1 = 0.0f;
    if (x < w && y < h) {
        const float mu1_sq = mu1 * mu1, mu2_sq = mu2 * mu2, mu12 = mu1 * mu2;
        const float s1 = eaa - mu1_sq, s2 = ebb - mu2_sq, s12 = eab - mu12;
        const float A1 = 2.0f * mu12 + kC1, A2 = 2.0f * s12 + kC2, B1 = mu1_sq + mu2_sq + kC1, B2 = s1 + s2 + kC2;
        const float inv = 1.0f / (B1 * B2);
        const float map = (A1 * A2) / (B1 * B2);
        v_ssim = map;
        v_l1 = fabsf(s_a[ty + kRadius][tx + kRadius] - s_b[ty + kRadius][tx + kRadius]);
        if (kGrad) {
            const float dS1 = -map / B2;
            const float dS12 = 2.0f * A1 * inv;
            const float dmu = 2.0f * mu2 * A2 * inv - 2.0f * mu1 * map / B1 - 2.0f * mu1 * dS1 - mu2 * dS12;
            const size_t p = plane + (size_t)y * w + x;
            planes[p] = dmu; planes[plane_floats + p] = dS1; planes[2 * plane_floats + p] = dS12;
        }
    }
    const float t_ssim = block_sum(v_ssim, s_red[0]);
    const float t_l1 = block_sum(v_l1, s_red[1]);
    if (tid == 0) {
        const size_t slot = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        slots[2 * slot] = t_l1; slots[2 * slot + 1] = t_ssim;
    }
}

// one workgroup per image: slots_per_image pairs -> out_l1[image], out_ssim[image]
__global__ void __launch_bounds__(kBlock)
photometric_finalise_kernel(const float* __restrict__ slots, int64_t slots_per_image, double inv_count, float* __restrict__ out_l1,
                            float* __restrict__ out_ssim) {
    __shared__ double s_sum[2][kBlock];
    const float* mine = slots + 2 * (size_t)blockIdx.x * slots_per_image;
    double l1 = 0.0, ss = 0.0;
    for (int64_t k = threadIdx.x; k < slots_per_image; k += kBlock) { l1 += (double)mine[2 * k]; ss += (double)mine[2 * k + 1]; }
    s_sum[0][threadIdx.x] = l1; s_sum[1][threadIdx.x] = ss;
    __syncthreads();
    for (int s = kBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) { s_sum[0][threadIdx.x] += s_sum[0][threadIdx.x + s]; s_sum[1][threadIdx.x] += s_sum[1][threadIdx.x + s]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { out_l1[blockIdx.x] = (float)(s_sum[0][0] * inv_count); out_ssim[blockIdx.x] = (float)(s_sum[1][0] * inv_count); }
}

__global__ void __launch_bounds__(kBlock)
photometric_backward_kernel(const float* __restrict__ img, const float* __restrict__ gt, int h, int w, int tiles_x, int channels,
                            Window win, const float* __restrict__ planes, size_t plane_floats, const float* __restrict__ g_l1,
                            const float* __restrict__ g_ssim, float inv_count, float* __restrict__ grad) {
    __shared__ float s_p[3][kHalo][kHalo];
    __shared__ float s_h[3][kHalo][kTile];
    const int tid = threadIdx.x;
    const int tile_x = blockIdx.x % tiles_x, tile_y = blockIdx.x / tiles_x;
    const size_t plane = (size_t)blockIdx.y * h * w;
    const int x0 = tile_x * kTile - kRadius, y0 = tile_y * kTile - kRadius;

    for (int k = tid; k < kHalo * kHalo; k += kBlock) {
        const int r = k / kHalo, c = k - r * kHalo;
        const int y = y0 + r, x = x0 + c;
        const bool in = y >= 0 && y < h && x >= 0 && x < w;
        const size_t p = plane + (size_t)(in ? y : 0) * w + (in ? x : 0);
        s_p[0][r][c] = in ? planes[p] : 0.0f;
        s_p[1][r][c] = in ? planes[plane_floats + p] : 0.0f;
        s_p[2][r][c] = in ? planes[2 * plane_floats + p] : 0.0f;
    }
    __syncthreads();
    for (int k = tid; k < kHalo * kTile; k += kBlock) {
        const int r = k / kTile, c = k - r * kTile;
        float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
            const float wt = win.w[t];
            s0 += wt * s_p[0][r][c + t]; s1 += wt * s_p[1][r][c + t]; s2 += wt * s_p[2][r][c + t];
        }
        s_h[0][r][c] = s0; s_h[1][r][c] = s1; s_h[2][r][c] = s2;
    }
    __syncthreads();

    const int tx = tid % kTile, ty = tid / kTile;
    const int x = tile_x * kTile + tx, y = tile_y * kTile + ty;
    if (x >= w || y >= h) return;
    float c_mu = 0.0f, c_s1 = 0.0f, c_s12 = 0.0f;
#pragma unroll
    for (int t = 0; t < kTaps; ++t) {
        const float wt = win.w[t];
        c_mu += wt * s_h[0][ty + t][tx]; c_s1 += wt * s_h[1][ty + t][tx]; c_s12 += wt * s_h[2][ty + t][tx];
    }
    const size_t p = plane + (size_t)y * w + x;
    const float a = img[p], b = gt[p];
    const int image = blockIdx.y / channels;
    const float diff = a - b;
    const float sgn = diff > 0.0f ? 1.0f : (diff < 0.0f ? -1.0f : 0.0f);
    const float d_ssim = c_mu + 2.0f * a * c_s1 + b * c_s12;
    grad[p] = g_l1[image] * sgn * inv_count + g_ssim[image] * d_ssim * inv_count;
}

}  // namespace

extern "C" {

int64_t pixie_photometric_workspace_bytes(int b, int c, int h, int w, int with_grad) {
    Layout L;
    if (make_layout(b, c, h, w, with_grad, L, "pixie_photometric_workspace_bytes")) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_photometric_forward(const float* d_img, const float* d_gt, int b, int c, int h, int w, void* d_workspace, int64_t workspace_bytes,
                              int with_grad, float* d_out_l1, float* d_out_ssim, void* stream) {
    Layout L;
    if (make_layout(b, c, h, w, with_grad, L, "pixie_photometric_forward")) return 1;
    PX_REQUIRE(d_img && d_gt && d_out_l1 && d_out_ssim, "pixie_photometric_forward: null pointer (both images and both outputs are required)");
    PX_REQUIRE(d_workspace && workspace_bytes >= (int64_t)L.total_bytes,
               "pixie_photometric_forward: workspace of %lld bytes is smaller than the %lld bytes that %d x %d x %d x %d %s gradient planes need",
               (long long)workspace_bytes, (long long)L.total_bytes, b, c, h, w, with_grad ? "with" : "without");
    PX_REQUIRE(((uintptr_t)d_workspace & 15) == 0, "pixie_photometric_forward: d_workspace must be 16-byte aligned");
    hipStream_t st = as_stream(stream);
    float* slots = (float*)d_workspace;
    float* planes = (float*)((char*)d_workspace + L.planes);
    const Window win = make_window();
    const dim3 grid((unsigned)(L.tiles_x * L.tiles_y), (unsigned)(b * c));
    if (with_grad)
        hipLaunchKernelGGL(photometric_forward_kernel<true>, grid, dim3(kBlock), 0, st, d_img, d_gt, h, w, L.tiles_x, win, slots, planes,
                           L.plane_floats);
    else
        hipLaunchKernelGGL(photometric_forward_kernel<false>, grid, dim3(kBlock), 0, st, d_img, d_gt, h, w, L.tiles_x, win, slots,
                           (float*)nullptr, L.plane_floats);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(photometric_finalise_kernel, dim3((unsigned)b), dim3(kBlock), 0, st, (const float*)slots, L.slots / b,
                       1.0 / ((double)c * h * w), d_out_l1, d_out_ssim);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_photometric_backward(const float* d_img, const float* d_gt, int b, int c, int h, int w, const void* d_workspace,
                               const float* d_g_l1, const float* d_g_ssim, float* d_grad_img, void* stream) {
    Layout L;
    if (make_layout(b, c, h, w, 1, L, "pixie_photometric_backward")) return 1;
    PX_REQUIRE(d_img && d_gt && d_workspace && d_g_l1 && d_g_ssim && d_grad_img,
               "pixie_photometric_backward: null pointer (images, workspace, both upstream gradients and the output are required)");
    hipStream_t st = as_stream(stream);
    const float* planes = (const float*)((const char*)d_workspace + L.planes);
    const Window win = make_window();
    const dim3 grid((unsigned)(L.tiles_x * L.tiles_y), (unsigned)(b * c));
    hipLaunchKernelGGL(photometric_backward_kernel, grid, dim3(kBlock), 0, st, d_img, d_gt, h, w, L.tiles_x, c, win, planes, L.plane_floats,
                       d_g_l1, d_g_ssim, (float)(1.0 / ((double)c * h * w)), d_grad_img);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
