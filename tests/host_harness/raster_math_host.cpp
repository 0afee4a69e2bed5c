// tests/host_harness/raster_math_host.cpp -- compiles pixie_amd/csrc/raster_math.h for the HOST so that CPU-only tests can check
// the rasteriser's per-Gaussian projection, its per-pixel blend and its spherical harmonics before any GPU run.
// Test infrastructure only: the product never executes this.
#include "../../pixie_amd/csrc/raster_math.h"
namespace rm = pixie::raster;
extern "C" {
// per Gaussian: out_f[p] = depth, px, py, conic a b c, cov2D is not kept; out_i[p] = radius, x0, y0, x1, y1 (radius 0: culled)
void hh_raster_project(int n, const float* means, const float* cov3d, const float* scales, const float* rotations, float scale_modifier,
                       const float* V, const float* P, float tanfovx, float tanfovy, int W, int H, float* out_f, int* out_i) {
    const rm::Camera cam = rm::make_camera(V, P, tanfovx, tanfovy, W, H);
    for (int p = 0; p < n; ++p) {
        float c6[6];
        if (cov3d) for (int d = 0; d < 6; ++d) c6[d] = cov3d[6 * p + d];
        else rm::cov3d_from_scale_rot(scales + 3 * p, scale_modifier, rotations + 4 * p, c6);
        rm::Splat2D o = {};
        const bool ok = rm::project(means + 3 * p, c6, cam, o);
        float* f = out_f + 6 * p;
        int* i = out_i + 5 * p;
        f[0] = ok ? o.depth : 0.f; f[1] = ok ? o.px : 0.f; f[2] = ok ? o.py : 0.f;
        f[3] = ok ? o.ca : 0.f; f[4] = ok ? o.cb : 0.f; f[5] = ok ? o.cc : 0.f;
        i[0] = o.radius; i[1] = ok ? o.x0 : 0; i[2] = ok ? o.y0 : 0; i[3] = ok ? o.x1 : 0; i[4] = ok ? o.y1 : 0;
    }
}
void hh_raster_cov3d(int n, const float* scales, const float* rotations, float scale_modifier, float* cov) {
    for (int p = 0; p < n; ++p) rm::cov3d_from_scale_rot(scales + 3 * p, scale_modifier, rotations + 4 * p, cov + 6 * p);
}
// one pixel over a sorted list: g[k] = gx, gy, conic a b c, opacity, r, g, b.  out = C(3) + T bg, T, last contributor
void hh_raster_blend(int n, const float* g, float pixx, float pixy, const float* bg, float* out) {
    rm::PixelAcc a = rm::pixel_start(false);
    for (int k = 0; k < n && !a.done; ++k) {
        const float* q = g + 9 * k;
        rm::blend(a, q[0], q[1], q[2], q[3], q[4], q[5], q[6], q[7], q[8], pixx, pixy);
    }
    out[0] = a.r + a.T * bg[0]; out[1] = a.g + a.T * bg[1]; out[2] = a.b + a.T * bg[2];
    out[3] = a.T; out[4] = (float)a.last;
}
void hh_raster_sh(int n, int k_coeffs, int degree, const float* shs, const float* dirs, float* rgb) {
    for (int p = 0; p < n; ++p) rm::sh_to_rgb(shs + (long)p * k_coeffs * 3, degree, dirs[3 * p], dirs[3 * p + 1], dirs[3 * p + 2], rgb + 3 * p);
}
}
