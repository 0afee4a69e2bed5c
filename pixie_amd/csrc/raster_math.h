// pixie_amd/csrc/raster_math.h -- per-Gaussian and per-sample arithmetic of the forward 3D Gaussian splatting rasteriser
// (Kerbl et al. 2023; EWA projection after Zwicker et al. 2002), as PG's frame loop uses it for inference
// (gs_simulation.py:610-619 -> diff-gaussian-rasterization forward).
//
// Register-level math, __host__ __device__ like splat_math.h: the kernels in raster.hip run it and
// tests/host_harness/raster_math_host.cpp checks it on the CPU.  Everything is float32, written from the published algorithm:
//   project():   near cull, EWA 2D covariance with the +0.3 low-pass, conic, 3-sigma radius, pixel centre, 16x16 tile rectangle
//   PixelAcc:    front-to-back alpha blending of one pixel with the 1/255 and 1e-4 rules
//   sh_to_rgb(): real spherical harmonics of degree 0..3 along the view direction, + 0.5, clamped at 0
// Matrices are in row-vector convention, [p, 1] . M, 16 floats in memory order (the reference's world_view_transform and
// full_proj_transform tensors as they lie in memory).
// Every array below is indexed with compile-time constants only, so nothing is spilled to scratch.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RASTER_HD __host__ __device__ __forceinline__
#else
#define RASTER_HD inline
#endif

namespace pixie {
namespace raster {

constexpr int kTile = 16;                 // tile edge in pixels; part of the result (a Gaussian reaches only the tiles of its rectangle)
constexpr float kNear = 0.2f;             // culled at p_view.z <= kNear
constexpr float kLowPass = 0.3f;          // added to both diagonal entries of the 2D covariance
constexpr float kAlphaMax = 0.99f;
constexpr float kAlphaMin = 1.0f / 255.0f;
constexpr float kTMin = 0.0001f;

struct Camera {
    float V[16], P[16];                   // view and full projection, row-vector convention
    float tanfovx, tanfovy, focal_x, focal_y;
    int W, H, tiles_x, tiles_y;
};

RASTER_HD Camera make_camera(const float* V, const float* P, float tanfovx, float tanfovy, int W, int H) {
    Camera c;
    for (int i = 0; i < 16; ++i) { c.V[i] = V[i]; c.P[i] = P[i]; }
    c.tanfovx = tanfovx; c.tanfovy = tanfovy;
    c.focal_x = (float)W / (2.0f * tanfovx);
    c.focal_y = (float)H / (2.0f * tanfovy);
    c.W = W; c.H = H;
    c.tiles_x = (W + kTile - 1) / kTile;
    c.tiles_y = (H + kTile - 1) / kTile;
    return c;
}

struct Splat2D {
    float depth, px, py;                  // p_view.z and the pixel centre
    float ca, cb, cc;                     // conic: inverse of the 2D covariance (a b; b c)
    int radius;
    int x0, y0, x1, y1;                   // tile rectangle [x0, x1) x [y0, y1)
};

// R S^2 R^T of a scale (times mod) and an un-normalised wxyz quaternion, as its 6-float upper triangle
RASTER_HD void cov3d_from_scale_rot(const float* s, float mod, const float* q, float* cov) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                        2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                        2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    const float s0 = mod * s[0], s1 = mod * s[1], s2 = mod * s[2];
    const float A[9] = {R[0] * s0, R[1] * s1, R[2] * s2, R[3] * s0, R[4] * s1, R[5] * s2, R[6] * s0, R[7] * s1, R[8] * s2};  // R S
    cov[0] = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
    cov[1] = A[0] * A[3] + A[1] * A[4] + A[2] * A[5];
    cov[2] = A[0] * A[6] + A[1] * A[7] + A[2] * A[8];
    cov[3] = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
    cov[4] = A[3] * A[6] + A[4] * A[7] + A[5] * A[8];
    cov[5] = A[6] * A[6] + A[7] * A[7] + A[8] * A[8];
}

// One edge of the tile rectangle: (int)(v / 16) clamped to [0, tiles], safe for any float v
RASTER_HD int tile_edge(float v, int tiles) {
    const float t = fminf(fmaxf(v / (float)kTile, 0.0f), (float)tiles);
    return (int)t;
}

RASTER_HD void tile_rect(float px, float py, int radius, int tiles_x, int tiles_y, int& x0, int& y0, int& x1, int& y1) {
    const float r = (float)radius;
    x0 = tile_edge(px - r, tiles_x);
    y0 = tile_edge(py - r, tiles_y);
    x1 = tile_edge(px + r + (float)(kTile - 1), tiles_x);
    y1 = tile_edge(py + r + (float)(kTile - 1), tiles_y);
}

// Projects one Gaussian.  false: it is culled (behind the near plane, singular 2D covariance, or no tile) and its radius is 0.
RASTER_HD bool project(const float* p, const float* cov, const Camera& c, Splat2D& o) {
    const float* V = c.V;
    const float* P = c.P;
    const float x = p[0], y = p[1], z = p[2];
    float tx = V[0] * x + V[4] * y + V[8] * z + V[12];
    float ty = V[1] * x + V[5] * y + V[9] * z + V[13];
    const float tz = V[2] * x + V[6] * y + V[10] * z + V[14];
    o.radius = 0;
    if (!(tz > kNear)) return false;
    const float hx = P[0] * x + P[4] * y + P[8] * z + P[12];
    const float hy = P[1] * x + P[5] * y + P[9] * z + P[13];
    const float hw = P[3] * x + P[7] * y + P[11] * z + P[15];
    const float pw = 1.0f / (hw + 0.0000001f);

    // EWA: J is the Jacobian of the perspective map at the (clamped) view-space centre, W the view rotation
    const float limx = 1.3f * c.tanfovx, limy = 1.3f * c.tanfovy;
    tx = fminf(limx, fmaxf(-limx, tx / tz)) * tz;
    ty = fminf(limy, fmaxf(-limy, ty / tz)) * tz;
    const float j00 = c.focal_x / tz, j02 = -(c.focal_x * tx) / (tz * tz);
    const float j11 = c.focal_y / tz, j12 = -(c.focal_y * ty) / (tz * tz);
    // rows of M = J W^T: M0k = j00 V[4k] + j02 V[4k+2], M1k = j11 V[4k+1] + j12 V[4k+2]
    const float m00 = j00 * V[0] + j02 * V[2], m01 = j00 * V[4] + j02 * V[6], m02 = j00 * V[8] + j02 * V[10];
    const float m10 = j11 * V[1] + j12 * V[2], m11 = j11 * V[5] + j12 * V[6], m12 = j11 * V[9] + j12 * V[10];
    // u = Sigma M0^T, v = Sigma M1^T
    const float u0 = cov[0] * m00 + cov[1] * m01 + cov[2] * m02;
    const float u1 = cov[1] * m00 + cov[3] * m01 + cov[4] * m02;
    const float u2 = cov[2] * m00 + cov[4] * m01 + cov[5] * m02;
    const float v0 = cov[0] * m10 + cov[1] * m11 + cov[2] * m12;
    const float v1 = cov[1] * m10 + cov[3] * m11 + cov[4] * m12;
    const float v2 = cov[2] * m10 + cov[4] * m11 + cov[5] * m12;
    const float a = m00 * u0 + m01 * u1 + m02 * u2 + kLowPass;
    const float b = m10 * u0 + m11 * u1 + m12 * u2;
    const float d = m10 * v0 + m11 * v1 + m12 * v2 + kLowPass;

    const float det = a * d - b * b;
    if (det == 0.0f) return false;
    const float det_inv = 1.0f / det;
    o.ca = d * det_inv;
    o.cb = -b * det_inv;
    o.cc = a * det_inv;

    const float mid = 0.5f * (a + d);
    const float disc = sqrtf(fmaxf(0.1f, mid * mid - det));
    const float lam = fmaxf(mid + disc, mid - disc);
    float rf = ceilf(3.0f * sqrtf(lam));
    if (!(rf < 1.0e9f)) rf = 1.0e9f;      // an overflowed or NaN extent covers the image; it must not overflow the int
    const int radius = (int)rf;
    o.px = ((hx * pw + 1.0f) * (float)c.W - 1.0f) * 0.5f;
    o.py = ((hy * pw + 1.0f) * (float)c.H - 1.0f) * 0.5f;
    tile_rect(o.px, o.py, radius, c.tiles_x, c.tiles_y, o.x0, o.y0, o.x1, o.y1);
    if ((o.x1 - o.x0) * (o.y1 - o.y0) == 0) return false;
    o.depth = tz;
    o.radius = radius;
    return true;
}

// One pixel's front-to-back accumulation
struct PixelAcc {
    float T, r, g, b;
    uint32_t seen, last;                  // instances visited / the last one that contributed
    bool done;
};

RASTER_HD PixelAcc pixel_start(bool done) {
    PixelAcc a;
    a.T = 1.0f; a.r = a.g = a.b = 0.0f; a.seen = a.last = 0u; a.done = done;
    return a;
}

// alpha of a Gaussian at a pixel, or a negative value where it does not contribute
RASTER_HD float sample_alpha(float gx, float gy, float ca, float cb, float cc, float opacity, float pixx, float pixy) {
    const float dx = gx - pixx, dy = gy - pixy;
    const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
    if (power > 0.0f) return -1.0f;
    const float alpha = fminf(kAlphaMax, opacity * expf(power));
    return alpha < kAlphaMin ? -1.0f : alpha;
}

RASTER_HD void blend(PixelAcc& a, float gx, float gy, float ca, float cb, float cc, float opacity, float cr, float cg, float cbl,
                     float pixx, float pixy) {
    a.seen++;
    const float alpha = sample_alpha(gx, gy, ca, cb, cc, opacity, pixx, pixy);
    if (alpha < 0.0f) return;
    const float test_T = a.T * (1.0f - alpha);
    if (test_T < kTMin) { a.done = true; return; }
    const float w = alpha * a.T;
    a.r += cr * w;
    a.g += cg * w;
    a.b += cbl * w;
    a.T = test_T;
    a.last = a.seen;
}

// Real spherical harmonics (degree 0..3) of `sh` ([K][3], K >= (degree+1)^2) along the unit vector (x, y, z), + 0.5, clamped at 0
RASTER_HD void sh_to_rgb(const float* sh, int degree, float x, float y, float z, float* rgb) {
    constexpr float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    constexpr float C20 = 1.0925484305920792f, C21 = -1.0925484305920792f, C22 = 0.31539156525252005f, C23 = -1.0925484305920792f,
                    C24 = 0.5462742152960396f;
    constexpr float C30 = -0.5900435899266435f, C31 = 2.890611442640554f, C32 = -0.4570457994644658f, C33 = 0.3731763325616595f,
                    C34 = -0.4570457994644658f, C35 = 1.445305721320277f, C36 = -0.5900435899266435f;
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    for (int ch = 0; ch < 3; ++ch) {
        float v = C0 * sh[ch];
        if (degree > 0) {
            v = v - C1 * y * sh[3 + ch] + C1 * z * sh[6 + ch] - C1 * x * sh[9 + ch];
            if (degree > 1) {
                v = v + C20 * xy * sh[12 + ch] + C21 * yz * sh[15 + ch] + C22 * (2.0f * zz - xx - yy) * sh[18 + ch]
                      + C23 * xz * sh[21 + ch] + C24 * (xx - yy) * sh[24 + ch];
                if (degree > 2) {
                    v = v + C30 * y * (3.0f * xx - yy) * sh[27 + ch] + C31 * xy * z * sh[30 + ch]
                          + C32 * y * (4.0f * zz - xx - yy) * sh[33 + ch] + C33 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * sh[36 + ch]
                          + C34 * x * (4.0f * zz - xx - yy) * sh[39 + ch] + C35 * z * (xx - yy) * sh[42 + ch]
                          + C36 * x * (xx - 3.0f * yy) * sh[45 + ch];
                }
            }
        }
        rgb[ch] = fmaxf(v + 0.5f, 0.0f);
    }
}

}  // namespace raster
}  // namespace pixie
