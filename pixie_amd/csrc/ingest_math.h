// pixie_amd/csrc/ingest_math.h -- per-Gaussian arithmetic of the scene ingest: everything PG/gs_simulation.py does to one Gaussian
// between GaussianModel.load_ply and fill_particles (:403-438).
//
// Register-level math, __host__ __device__ like raster_math.h and splat_math.h: the kernels in scene_ingest.hip run it and
// tests/host_harness/ingest_math_host.cpp checks it on the CPU.  Everything is float32, in the reference's order of operations:
//   activate_opacity()   sigmoid                                                        (GaussianModel.get_opacity)
//   covariance()         exp(scale), quaternion / |quaternion| -> R, (R S)(R S)^T, 6 upper entries 00 01 02 11 12 22
//                                                                                       (get_covariance, general_utils.py:64-110)
//   rotate_position()    p @ R_0^T @ R_1^T ...                                          (apply_rotations)
//   rotate_covariance()  R_k (S R_k^T), k in order                                      (apply_cov_rotations)
//   classify()           0 dropped / 1 selected / 2 unselected                          (:405, :423-424)
//   frame_of_bounds()    mean = (min + max) / 2, scale = 1 / max(max - min)             (transform2origin)
//   map_position()       ((p - mean) * scale + 1) + (0, 0, z_shift)                     (transform2origin, shift2center111)
//   map_covariance()     S * (scale * scale)                                            (:438)
// Built with -ffp-contract=off on both sides, so the device and the host round identically apart from expf.  The one fused
// accumulation is written out: rotate_position() sums its three products with fmaf, as the BLAS kernel behind the reference's
// torch.mm does (fmaf is correctly rounded on both sides, so the bits still agree).  Unfused, the bounding box -- hence scale and mean,
// which every selected position inherits -- sat up to an ulp further from the float64 run than the reference's own float32 run does.
// Rotation matrices are row-major, 9 floats each, one after the other.  Arrays are indexed with compile-time constants only.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define INGEST_HD __host__ __device__ __forceinline__
#else
#define INGEST_HD inline
#endif

namespace pixie {
namespace ingest {

constexpr int kMaxRotations = 8;
enum { kDropped = 0, kSelected = 1, kUnselected = 2 };

INGEST_HD float activate_opacity(float raw) { return 1.0f / (1.0f + expf(-raw)); }

// log-scales and an un-normalised wxyz quaternion -> the 6 upper entries of (R S)(R S)^T
INGEST_HD void covariance(const float* log_scale, const float* quat, float* c6) {
    const float norm = sqrtf(quat[0] * quat[0] + quat[1] * quat[1] + quat[2] * quat[2] + quat[3] * quat[3]);
    const float r = quat[0] / norm, x = quat[1] / norm, y = quat[2] / norm, z = quat[3] / norm;
    const float R[9] = {1.f - 2.f * (y * y + z * z), 2.f * (x * y - r * z), 2.f * (x * z + r * y),
                        2.f * (x * y + r * z), 1.f - 2.f * (x * x + z * z), 2.f * (y * z - r * x),
                        2.f * (x * z - r * y), 2.f * (y * z + r * x), 1.f - 2.f * (x * x + y * y)};
    const float s0 = expf(log_scale[0]), s1 = expf(log_scale[1]), s2 = expf(log_scale[2]);
    const float A[9] = {R[0] * s0, R[1] * s1, R[2] * s2, R[3] * s0, R[4] * s1, R[5] * s2, R[6] * s0, R[7] * s1, R[8] * s2};  // R S
    c6[0] = A[0] * A[0] + A[1] * A[1] + A[2] * A[2];
    c6[1] = A[0] * A[3] + A[1] * A[4] + A[2] * A[5];
    c6[2] = A[0] * A[6] + A[1] * A[7] + A[2] * A[8];
    c6[3] = A[3] * A[3] + A[4] * A[4] + A[5] * A[5];
    c6[4] = A[3] * A[6] + A[4] * A[7] + A[5] * A[8];
    c6[5] = A[6] * A[6] + A[7] * A[7] + A[8] * A[8];
}

// p @ R_0^T @ R_1^T ... ; `rot` holds n_rot matrices.  One rounded product, then two fused multiply-adds per component.
INGEST_HD void rotate_position(const float* p, const float* rot, int n_rot, float* out) {
    float a = p[0], b = p[1], c = p[2];
    for (int k = 0; k < n_rot; ++k) {
        const float* R = rot + 9 * k;
        const float na = fmaf(c, R[2], fmaf(b, R[1], a * R[0]));
        const float nb = fmaf(c, R[5], fmaf(b, R[4], a * R[3]));
        const float nc = fmaf(c, R[8], fmaf(b, R[7], a * R[6]));
        a = na; b = nb; c = nc;
    }
    out[0] = a; out[1] = b; out[2] = c;
}

// R_k (S R_k^T) for k in order, on the full symmetric matrix as the reference does; the 6 upper entries come back
INGEST_HD void rotate_covariance(const float* c6, const float* rot, int n_rot, float* out) {
    float s00 = c6[0], s01 = c6[1], s02 = c6[2], s10 = c6[1], s11 = c6[3], s12 = c6[4], s20 = c6[2], s21 = c6[4], s22 = c6[5];
    for (int k = 0; k < n_rot; ++k) {
        const float* R = rot + 9 * k;
        // T = S R^T
        const float t00 = s00 * R[0] + s01 * R[1] + s02 * R[2], t01 = s00 * R[3] + s01 * R[4] + s02 * R[5], t02 = s00 * R[6] + s01 * R[7] + s02 * R[8];
        const float t10 = s10 * R[0] + s11 * R[1] + s12 * R[2], t11 = s10 * R[3] + s11 * R[4] + s12 * R[5], t12 = s10 * R[6] + s11 * R[7] + s12 * R[8];
        const float t20 = s20 * R[0] + s21 * R[1] + s22 * R[2], t21 = s20 * R[3] + s21 * R[4] + s22 * R[5], t22 = s20 * R[6] + s21 * R[7] + s22 * R[8];
        // S = R T
        s00 = R[0] * t00 + R[1] * t10 + R[2] * t20; s01 = R[0] * t01 + R[1] * t11 + R[2] * t21; s02 = R[0] * t02 + R[1] * t12 + R[2] * t22;
        s10 = R[3] * t00 + R[4] * t10 + R[5] * t20; s11 = R[3] * t01 + R[4] * t11 + R[5] * t21; s12 = R[3] * t02 + R[4] * t12 + R[5] * t22;
        s20 = R[6] * t00 + R[7] * t10 + R[8] * t20; s21 = R[6] * t01 + R[7] * t11 + R[8] * t21; s22 = R[6] * t02 + R[7] * t12 + R[8] * t22;
    }
    out[0] = s00; out[1] = s01; out[2] = s02; out[3] = s11; out[4] = s12; out[5] = s22;
}

// The class of one Gaussian from its ACTIVATED opacity and ROTATED position.  `area` = (x0, x1, y0, y1, z0, z1) or NULL for no
// sim_area (then nothing is unselected).  Strict inequalities, float32 compares, as the reference's masks.
INGEST_HD int classify(float opacity, const float* rotated, float opacity_threshold, const float* area) {
    if (!(opacity > opacity_threshold)) return kDropped;
    if (!area) return kSelected;
    const bool in = rotated[0] > area[0] && rotated[0] < area[1] && rotated[1] > area[2] && rotated[1] < area[3] &&
                    rotated[2] > area[4] && rotated[2] < area[5];
    return in ? kSelected : kUnselected;
}

// transform2origin's frame from the bounding box of the selected rotated positions; returns max(max - min)
INGEST_HD float frame_of_bounds(const float* lo, const float* hi, float* mean, float* scale) {
    const float dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    const float max_diff = fmaxf(fmaxf(dx, dy), dz);
    mean[0] = (lo[0] + hi[0]) / 2.0f;
    mean[1] = (lo[1] + hi[1]) / 2.0f;
    mean[2] = (lo[2] + hi[2]) / 2.0f;
    *scale = 1.0f / max_diff;
    return max_diff;
}

// solver-frame position; the two additions of shift2center111 are kept apart (x and y add an exact 0)
INGEST_HD void map_position(const float* rotated, const float* mean, float scale, float z_shift, float* out) {
    out[0] = (rotated[0] - mean[0]) * scale + 1.0f;
    out[1] = (rotated[1] - mean[1]) * scale + 1.0f;
    out[2] = ((rotated[2] - mean[2]) * scale + 1.0f) + z_shift;
}

INGEST_HD void map_covariance(const float* rotated_c6, float scale, float* out) {
    const float s2 = scale * scale;
    out[0] = rotated_c6[0] * s2; out[1] = rotated_c6[1] * s2; out[2] = rotated_c6[2] * s2;
    out[3] = rotated_c6[3] * s2; out[4] = rotated_c6[4] * s2; out[5] = rotated_c6[5] * s2;
}

}  // namespace ingest
}  // namespace pixie
