// pixie_amd/csrc/raster_grad_math.h -- the derivative of raster_math.h: per-sample and per-Gaussian arithmetic of the backward pass of
// the 3D Gaussian splatting rasteriser.
//
// The gradient is the exact derivative of the forward as include/pixie_hip.h section D defines it, with every discrete decision held
// fixed: culling, radius, tile rectangle, order, the power > 0 / 1/255 / 1e-4 rules, min(0.99, .) and the two clamps of project() and
// sh_to_rgb() taking whichever branch they took.  Register-level math, __host__ __device__ and float32 like raster_math.h: the kernels
// in raster_backward.hip run it and tests/host_harness/raster_grad_math_host.cpp checks it on the CPU.
//   sample_backward():        one Gaussian at one pixel -> its nine partials (centre 2, conic 3, opacity 1, colour 3)
//   project_backward():       dL/dcentre, dL/dconic -> dL/dcov3D (6) and dL/dmean3D, through the EWA projection
//   cov3d_backward():         dL/dcov3D -> dL/dscales, dL/drotations
//   sh_backward():            dL/dcolour -> dL/dshs and dL/d(view direction); direction_backward() carries that to the mean
// The blend is walked front to back with the forward's own operations, so T and the accumulated colour have the forward's bits; what
// lies behind a sample is the pixel's final colour minus what has been accumulated up to and including it, which contains the
// background term final_T * bg.
// Every array below is indexed with compile-time constants only, so nothing is spilled to scratch.
#pragma once
#include "raster_math.h"

namespace pixie {
namespace raster {

constexpr int kSampleGrads = 9;           // centre x y, conic a b c, opacity, colour r g b

// The walk of one pixel: the forward's accumulation (same bits) plus what the backward needs of the pixel.
struct PixelGradWalk {
    float T, r, g, b;                     // as PixelAcc, before the next sample
    float out_r, out_g, out_b;            // the pixel's colour as the forward wrote it (C + final_T * bg)
    float gr, gg, gb;                     // dL/dcolour of the pixel
};

// One sample.  false: the Gaussian does not contribute to the pixel (the decision of sample_alpha, bit for bit) and `d` is untouched.
// Otherwise d[0..8] = this sample's share of dL/d(centre x, centre y, conic a, b, c, opacity, colour r, g, b) and the walk advances.
// The caller guarantees what the forward's n_contrib says: that the sample lies before the pixel's last contributor or is it.
RASTER_HD bool sample_backward(PixelGradWalk& w, float gx, float gy, float ca, float cb, float cc, float opacity, float cr, float cg,
                               float cbl, float pixx, float pixy, float* d) {
    const float alpha = sample_alpha(gx, gy, ca, cb, cc, opacity, pixx, pixy);
    if (alpha < 0.0f) return false;
    const float dx = gx - pixx, dy = gy - pixy;
    const float power = -0.5f * (ca * dx * dx + cc * dy * dy) - cb * dx * dy;
    const float G = expf(power);
    const float raw = opacity * G;
    const float T = w.T;
    const float wt = alpha * T;
    w.r += cr * wt;                       // the forward's blend(), operation for operation
    w.g += cg * wt;
    w.b += cbl * wt;
    w.T = T * (1.0f - alpha);
    d[6] = w.gr * wt;
    d[7] = w.gg * wt;
    d[8] = w.gb * wt;
    // colour = ... + alpha T c + (1 - alpha) * (what lies behind) / (1 - alpha)
    const float behind = w.gr * (w.out_r - w.r) + w.gg * (w.out_g - w.g) + w.gb * (w.out_b - w.b);
    const float here = w.gr * cr + w.gg * cg + w.gb * cbl;
    float dalpha = T * here - behind / (1.0f - alpha);
    if (raw > kAlphaMax) dalpha = 0.0f;   // min(0.99, .) took the constant
    d[5] = G * dalpha;
    const float dpower = raw * dalpha;
    d[0] = dpower * (-ca * dx - cb * dy);
    d[1] = dpower * (-cc * dy - cb * dx);
    d[2] = dpower * (-0.5f * dx * dx);
    d[3] = dpower * (-(dx * dy));
    d[4] = dpower * (-0.5f * dy * dy);
    return true;
}

// dL/d(pixel centre) (dcentre), dL/dconic -> dcov[6] (written) and dmean[3] (accumulated into).  The Gaussian must be one project()
// accepted; the intermediates are recomputed with project()'s expressions.
RASTER_HD void project_backward(const float* p, const float* cov, const Camera& c, const float* dcentre, const float* dconic, float* dcov,
                                float* dmean) {
    const float* V = c.V;
    const float* P = c.P;
    const float x = p[0], y = p[1], z = p[2];
    const float tx = V[0] * x + V[4] * y + V[8] * z + V[12];
    const float ty = V[1] * x + V[5] * y + V[9] * z + V[13];
    const float tz = V[2] * x + V[6] * y + V[10] * z + V[14];
    const float hx = P[0] * x + P[4] * y + P[8] * z + P[12];
    const float hy = P[1] * x + P[5] * y + P[9] * z + P[13];
    const float hw = P[3] * x + P[7] * y + P[11] * z + P[15];
    const float pw = 1.0f / (hw + 0.0000001f);

    const float limx = 1.3f * c.tanfovx, limy = 1.3f * c.tanfovy;
    const float rx = tx / tz, ry = ty / tz;
    const bool free_x = !(rx > limx) && !(rx < -limx), free_y = !(ry > limy) && !(ry < -limy);
    const float txc = fminf(limx, fmaxf(-limx, rx)) * tz;
    const float tyc = fminf(limy, fmaxf(-limy, ry)) * tz;
    const float tz2 = tz * tz, tz3 = tz2 * tz;
    const float j00 = c.focal_x / tz, j02 = -(c.focal_x * txc) / tz2;
    const float j11 = c.focal_y / tz, j12 = -(c.focal_y * tyc) / tz2;
    const float m00 = j00 * V[0] + j02 * V[2], m01 = j00 * V[4] + j02 * V[6], m02 = j00 * V[8] + j02 * V[10];
    const float m10 = j11 * V[1] + j12 * V[2], m11 = j11 * V[5] + j12 * V[6], m12 = j11 * V[9] + j12 * V[10];
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
    const float inv = 1.0f / det;

    // conic = (d, -b, a) / det
    const float s = (dconic[0] * d - dconic[1] * b + dconic[2] * a) * (inv * inv);
    const float da = dconic[2] * inv - s * d;
    const float db = -dconic[1] * inv + 2.0f * s * b;
    const float dd = dconic[0] * inv - s * a;

    // a = M0 S M0^T + 0.3, b = M1 S M0^T, d = M1 S M1^T + 0.3
    dcov[0] = da * m00 * m00 + db * m00 * m10 + dd * m10 * m10;
    dcov[3] = da * m01 * m01 + db * m01 * m11 + dd * m11 * m11;
    dcov[5] = da * m02 * m02 + db * m02 * m12 + dd * m12 * m12;
    dcov[1] = 2.0f * da * m00 * m01 + db * (m00 * m11 + m01 * m10) + 2.0f * dd * m10 * m11;
    dcov[2] = 2.0f * da * m00 * m02 + db * (m00 * m12 + m02 * m10) + 2.0f * dd * m10 * m12;
    dcov[4] = 2.0f * da * m01 * m02 + db * (m01 * m12 + m02 * m11) + 2.0f * dd * m11 * m12;

    const float dm00 = 2.0f * da * u0 + db * v0, dm01 = 2.0f * da * u1 + db * v1, dm02 = 2.0f * da * u2 + db * v2;
    const float dm10 = db * u0 + 2.0f * dd * v0, dm11 = db * u1 + 2.0f * dd * v1, dm12 = db * u2 + 2.0f * dd * v2;
    const float dj00 = dm00 * V[0] + dm01 * V[4] + dm02 * V[8];
    const float dj02 = dm00 * V[2] + dm01 * V[6] + dm02 * V[10];
    const float dj11 = dm10 * V[1] + dm11 * V[5] + dm12 * V[9];
    const float dj12 = dm10 * V[2] + dm11 * V[6] + dm12 * V[10];
    // j02 = -focal_x tx / tz^2 where the clamp is idle, -focal_x (+-limx) / tz where it is active; the same in y
    const float dtx = free_x ? -(c.focal_x / tz2) * dj02 : 0.0f;
    const float dty = free_y ? -(c.focal_y / tz2) * dj12 : 0.0f;
    const float dtz = -(c.focal_x / tz2) * dj00 - (c.focal_y / tz2) * dj11
                      + (free_x ? 2.0f : 1.0f) * (c.focal_x * txc / tz3) * dj02 + (free_y ? 2.0f : 1.0f) * (c.focal_y * tyc / tz3) * dj12;

    // the centre: px = ((hx pw + 1) W - 1) / 2
    const float dndx = dcentre[0] * (0.5f * (float)c.W), dndy = dcentre[1] * (0.5f * (float)c.H);
    const float dhx = dndx * pw, dhy = dndy * pw;
    const float dhw = -(pw * pw) * (dndx * hx + dndy * hy);

    dmean[0] += V[0] * dtx + V[1] * dty + V[2] * dtz + P[0] * dhx + P[1] * dhy + P[3] * dhw;
    dmean[1] += V[4] * dtx + V[5] * dty + V[6] * dtz + P[4] * dhx + P[5] * dhy + P[7] * dhw;
    dmean[2] += V[8] * dtx + V[9] * dty + V[10] * dtz + P[8] * dhx + P[9] * dhy + P[11] * dhw;
}

// dL/dcov3D (6, one entry per upper-triangle parameter) -> dL/dscales (carrying `mod`) and dL/drotations (un-normalised wxyz)
RASTER_HD void cov3d_backward(const float* s, float mod, const float* q, const float* dcov, float* ds, float* dq) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                        2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                        2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    const float s0 = mod * s[0], s1 = mod * s[1], s2 = mod * s[2];
    const float A[9] = {R[0] * s0, R[1] * s1, R[2] * s2, R[3] * s0, R[4] * s1, R[5] * s2, R[6] * s0, R[7] * s1, R[8] * s2};
    // cov_ij = sum_k A_ik A_jk: dA = Gs A with Gs symmetric, 2 dcov on the diagonal and dcov off it
    const float g00 = 2.f * dcov[0], g01 = dcov[1], g02 = dcov[2], g11 = 2.f * dcov[3], g12 = dcov[4], g22 = 2.f * dcov[5];
    const float dA[9] = {g00 * A[0] + g01 * A[3] + g02 * A[6], g00 * A[1] + g01 * A[4] + g02 * A[7], g00 * A[2] + g01 * A[5] + g02 * A[8],
                         g01 * A[0] + g11 * A[3] + g12 * A[6], g01 * A[1] + g11 * A[4] + g12 * A[7], g01 * A[2] + g11 * A[5] + g12 * A[8],
                         g02 * A[0] + g12 * A[3] + g22 * A[6], g02 * A[1] + g12 * A[4] + g22 * A[7], g02 * A[2] + g12 * A[5] + g22 * A[8]};
    ds[0] = mod * (dA[0] * R[0] + dA[3] * R[3] + dA[6] * R[6]);
    ds[1] = mod * (dA[1] * R[1] + dA[4] * R[4] + dA[7] * R[7]);
    ds[2] = mod * (dA[2] * R[2] + dA[5] * R[5] + dA[8] * R[8]);
    const float dR[9] = {dA[0] * s0, dA[1] * s1, dA[2] * s2, dA[3] * s0, dA[4] * s1, dA[5] * s2, dA[6] * s0, dA[7] * s1, dA[8] * s2};
    dq[0] = 2.f * (-z * dR[1] + y * dR[2] + z * dR[3] - x * dR[5] - y * dR[6] + x * dR[7]);
    dq[1] = 2.f * (y * dR[1] + z * dR[2] + y * dR[3] - 2.f * x * dR[4] - r * dR[5] + z * dR[6] + r * dR[7] - 2.f * x * dR[8]);
    dq[2] = 2.f * (-2.f * y * dR[0] + x * dR[1] + r * dR[2] + x * dR[3] + z * dR[5] - r * dR[6] + z * dR[7] - 2.f * y * dR[8]);
    dq[3] = 2.f * (-2.f * z * dR[0] - r * dR[1] + x * dR[2] + r * dR[3] - 2.f * z * dR[4] + y * dR[5] + x * dR[6] + y * dR[7]);
}

// dL/dcolour (3) -> dsh ([(degree+1)^2][3], written where not null) and ddir (3, written): the derivative of sh_to_rgb along the unit vector
// (x, y, z), treating x, y and z as independent.  Zero for a channel whose max(., 0) clamp is active.
RASTER_HD void sh_backward(const float* sh, int degree, float x, float y, float z, const float* dcol, float* dsh, float* ddir) {
    constexpr float C0 = 0.28209479177387814f, C1 = 0.4886025119029199f;
    constexpr float C20 = 1.0925484305920792f, C21 = -1.0925484305920792f, C22 = 0.31539156525252005f, C23 = -1.0925484305920792f,
                    C24 = 0.5462742152960396f;
    constexpr float C30 = -0.5900435899266435f, C31 = 2.890611442640554f, C32 = -0.4570457994644658f, C33 = 0.3731763325616595f,
                    C34 = -0.4570457994644658f, C35 = 1.445305721320277f, C36 = -0.5900435899266435f;
    float rgb[3];
    sh_to_rgb(sh, degree, x, y, z, rgb);
    const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
    float ax = 0.0f, ay = 0.0f, az = 0.0f;
    for (int ch = 0; ch < 3; ++ch) {
        const float dv = rgb[ch] > 0.0f ? dcol[ch] : 0.0f;
        if (dsh) dsh[ch] = C0 * dv;
        if (degree > 0) {
            if (dsh) dsh[3 + ch] = -C1 * y * dv;
            if (dsh) dsh[6 + ch] = C1 * z * dv;
            if (dsh) dsh[9 + ch] = -C1 * x * dv;
            float gx = -C1 * sh[9 + ch], gy = -C1 * sh[3 + ch], gz = C1 * sh[6 + ch];
            if (degree > 1) {
                if (dsh) dsh[12 + ch] = C20 * xy * dv;
                if (dsh) dsh[15 + ch] = C21 * yz * dv;
                if (dsh) dsh[18 + ch] = C22 * (2.0f * zz - xx - yy) * dv;
                if (dsh) dsh[21 + ch] = C23 * xz * dv;
                if (dsh) dsh[24 + ch] = C24 * (xx - yy) * dv;
                gx += C20 * y * sh[12 + ch] - 2.0f * C22 * x * sh[18 + ch] + C23 * z * sh[21 + ch] + 2.0f * C24 * x * sh[24 + ch];
                gy += C20 * x * sh[12 + ch] + C21 * z * sh[15 + ch] - 2.0f * C22 * y * sh[18 + ch] - 2.0f * C24 * y * sh[24 + ch];
                gz += C21 * y * sh[15 + ch] + 4.0f * C22 * z * sh[18 + ch] + C23 * x * sh[21 + ch];
                if (degree > 2) {
                    if (dsh) dsh[27 + ch] = C30 * y * (3.0f * xx - yy) * dv;
                    if (dsh) dsh[30 + ch] = C31 * xy * z * dv;
                    if (dsh) dsh[33 + ch] = C32 * y * (4.0f * zz - xx - yy) * dv;
                    if (dsh) dsh[36 + ch] = C33 * z * (2.0f * zz - 3.0f * xx - 3.0f * yy) * dv;
                    if (dsh) dsh[39 + ch] = C34 * x * (4.0f * zz - xx - yy) * dv;
                    if (dsh) dsh[42 + ch] = C35 * z * (xx - yy) * dv;
                    if (dsh) dsh[45 + ch] = C36 * x * (xx - 3.0f * yy) * dv;
                    gx += C30 * 6.0f * xy * sh[27 + ch] + C31 * yz * sh[30 + ch] - C32 * 2.0f * xy * sh[33 + ch] - C33 * 6.0f * xz * sh[36 + ch]
                          + C34 * (4.0f * zz - 3.0f * xx - yy) * sh[39 + ch] + C35 * 2.0f * xz * sh[42 + ch] + C36 * (3.0f * xx - 3.0f * yy) * sh[45 + ch];
                    gy += C30 * (3.0f * xx - 3.0f * yy) * sh[27 + ch] + C31 * xz * sh[30 + ch] + C32 * (4.0f * zz - xx - 3.0f * yy) * sh[33 + ch]
                          - C33 * 6.0f * yz * sh[36 + ch] - C34 * 2.0f * xy * sh[39 + ch] - C35 * 2.0f * yz * sh[42 + ch] - C36 * 6.0f * xy * sh[45 + ch];
                    gz += C31 * xy * sh[30 + ch] + C32 * 8.0f * yz * sh[33 + ch] + C33 * (6.0f * zz - 3.0f * xx - 3.0f * yy) * sh[36 + ch]
                          + C34 * 8.0f * xz * sh[39 + ch] + C35 * (xx - yy) * sh[42 + ch];
                }
            }
            ax += gx * dv;
            ay += gy * dv;
            az += gz * dv;
        }
    }
    ddir[0] = ax; ddir[1] = ay; ddir[2] = az;
}

// dir = v / |v|: dL/ddir -> accumulated into dv (the mean)
RASTER_HD void direction_backward(float vx, float vy, float vz, const float* ddir, float* dv) {
    const float len = sqrtf(vx * vx + vy * vy + vz * vz);
    const float x = vx / len, y = vy / len, z = vz / len;
    const float along = x * ddir[0] + y * ddir[1] + z * ddir[2];
    dv[0] += (ddir[0] - x * along) / len;
    dv[1] += (ddir[1] - y * along) / len;
    dv[2] += (ddir[2] - z * along) / len;
}

}  // namespace raster
}  // namespace pixie
