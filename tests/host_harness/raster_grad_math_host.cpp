// tests/host_harness/raster_grad_math_host.cpp -- compiles pixie_amd/csrc/raster_grad_math.h for the HOST so that a CPU-only test can
// check the rasteriser's backward arithmetic on whole small scenes before any GPU run.
// Test infrastructure only: the product never executes this.
//
// A plain loop, no tiling: project every Gaussian, order the survivors by (depth, index), blend every pixel over the Gaussians whose
// tile rectangle holds the pixel's tile (the forward, raster_math.h), then walk every pixel again with sample_backward and add the
// nine float32 partials of every sample to its Gaussian, and last apply the per-Gaussian chain.  The driver's own sum over pixels
// is kept in double: it stands for the kernels' tree-shaped reduction and is not what is under test, the float32 values summed are.
#include <algorithm>
#include <vector>

#include "../../pixie_amd/csrc/raster_grad_math.h"
namespace rm = pixie::raster;

extern "C" {
// Inputs as pixie_raster_forward takes them (cov3d or scales + rotations; colors or shs at sh_degree from campos), w = dL/dcolour
// [3][H][W].  Outputs, each written for all n Gaussians: out_color [3][H][W]; d_means3d [n][3], d_means2d [n][3], d_opacity [n],
// d_colors [n][3], d_shs [n][sh_k][3] (with shs), d_cov [n][6] (with cov3d) or d_scales [n][3] and d_rots [n][4].
// Returns the largest n_contrib of the image.
int hh_raster_grad(int n, const float* means, const float* cov3d, const float* scales, const float* rots, float mod, const float* opacity,
                   const float* colors, const float* shs, int sh_k, int sh_degree, const float* campos, const float* V, const float* P,
                   float tanfovx, float tanfovy, int W, int H, const float* bg, const float* w, float* out_color, float* d_means3d,
                   float* d_means2d, float* d_opacity, float* d_colors, float* d_shs, float* d_cov, float* d_scales, float* d_rots) {
    const rm::Camera cam = rm::make_camera(V, P, tanfovx, tanfovy, W, H);
    std::vector<rm::Splat2D> sp(n);
    std::vector<float> c6(6 * (size_t)n), rgb(3 * (size_t)n);
    std::vector<int> order;
    for (int p = 0; p < n; ++p) {
        if (cov3d) for (int d = 0; d < 6; ++d) c6[6 * p + d] = cov3d[6 * p + d];
        else rm::cov3d_from_scale_rot(scales + 3 * p, mod, rots + 4 * p, &c6[6 * p]);
        sp[p] = rm::Splat2D{};
        if (rm::project(means + 3 * p, &c6[6 * p], cam, sp[p])) order.push_back(p);
        if (shs) {
            const float dx = means[3 * p] - campos[0], dy = means[3 * p + 1] - campos[1], dz = means[3 * p + 2] - campos[2];
            const float len = sqrtf(dx * dx + dy * dy + dz * dz);
            rm::sh_to_rgb(shs + (size_t)p * sh_k * 3, sh_degree, dx / len, dy / len, dz / len, &rgb[3 * p]);
        } else {
            for (int d = 0; d < 3; ++d) rgb[3 * p + d] = colors[3 * p + d];
        }
    }
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return sp[a].depth < sp[b].depth; });
    std::vector<double> part(9 * (size_t)n, 0.0);
    const size_t plane = (size_t)W * H;
    int reach = 0;
    for (int py = 0; py < H; ++py)
        for (int px = 0; px < W; ++px) {
            const int tx = px / rm::kTile, ty = py / rm::kTile;
            const float fx = (float)px, fy = (float)py;
            const size_t pix = (size_t)py * W + px;
            rm::PixelAcc acc = rm::pixel_start(false);
            for (size_t k = 0; k < order.size() && !acc.done; ++k) {
                const int g = order[k];
                const rm::Splat2D& s = sp[g];
                if (tx < s.x0 || tx >= s.x1 || ty < s.y0 || ty >= s.y1) continue;
                rm::blend(acc, s.px, s.py, s.ca, s.cb, s.cc, opacity[g], rgb[3 * g], rgb[3 * g + 1], rgb[3 * g + 2], fx, fy);
            }
            out_color[pix] = acc.r + acc.T * bg[0];
            out_color[plane + pix] = acc.g + acc.T * bg[1];
            out_color[2 * plane + pix] = acc.b + acc.T * bg[2];
            if ((int)acc.last > reach) reach = (int)acc.last;
            rm::PixelGradWalk walk;
            walk.T = 1.0f; walk.r = walk.g = walk.b = 0.0f;
            walk.out_r = out_color[pix]; walk.out_g = out_color[plane + pix]; walk.out_b = out_color[2 * plane + pix];
            walk.gr = w[pix]; walk.gg = w[plane + pix]; walk.gb = w[2 * plane + pix];
            uint32_t seen = 0;
            for (size_t k = 0; k < order.size() && seen < acc.last; ++k) {
                const int g = order[k];
                const rm::Splat2D& s = sp[g];
                if (tx < s.x0 || tx >= s.x1 || ty < s.y0 || ty >= s.y1) continue;
                ++seen;
                float d[rm::kSampleGrads];
                if (rm::sample_backward(walk, s.px, s.py, s.ca, s.cb, s.cc, opacity[g], rgb[3 * g], rgb[3 * g + 1], rgb[3 * g + 2], fx, fy, d))
                    for (int q = 0; q < rm::kSampleGrads; ++q) part[9 * (size_t)g + q] += (double)d[q];
            }
        }
    for (int p = 0; p < n; ++p) {
        float s[rm::kSampleGrads];
        for (int q = 0; q < rm::kSampleGrads; ++q) s[q] = (float)part[9 * (size_t)p + q];
        const bool live = sp[p].radius > 0;
        float dmean[3] = {0.f, 0.f, 0.f}, dcov[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, ds[3] = {0.f, 0.f, 0.f}, dq[4] = {0.f, 0.f, 0.f, 0.f};
        if (shs) {
            float* dsh = d_shs + (size_t)p * sh_k * 3;
            for (int k = 0; k < sh_k * 3; ++k) dsh[k] = 0.f;
            if (live) {
                const float vx = means[3 * p] - campos[0], vy = means[3 * p + 1] - campos[1], vz = means[3 * p + 2] - campos[2];
                const float len = sqrtf(vx * vx + vy * vy + vz * vz);
                float ddir[3];
                rm::sh_backward(shs + (size_t)p * sh_k * 3, sh_degree, vx / len, vy / len, vz / len, s + 6, dsh, ddir);
                rm::direction_backward(vx, vy, vz, ddir, dmean);
            }
        }
        if (live) {
            rm::project_backward(means + 3 * p, &c6[6 * p], cam, s, s + 2, dcov, dmean);
            if (!cov3d) rm::cov3d_backward(scales + 3 * p, mod, rots + 4 * p, dcov, ds, dq);
        }
        for (int d = 0; d < 3; ++d) d_means3d[3 * p + d] = dmean[d];
        d_means2d[3 * p] = s[0] * (0.5f * (float)W);
        d_means2d[3 * p + 1] = s[1] * (0.5f * (float)H);
        d_means2d[3 * p + 2] = 0.f;
        d_opacity[p] = s[5];
        for (int d = 0; d < 3; ++d) d_colors[3 * p + d] = s[6 + d];
        if (cov3d) for (int d = 0; d < 6; ++d) d_cov[6 * p + d] = dcov[d];
        else {
            for (int d = 0; d < 3; ++d) d_scales[3 * p + d] = ds[d];
            for (int d = 0; d < 4; ++d) d_rots[4 * p + d] = dq[d];
        }
    }
    return reach;
}
}
