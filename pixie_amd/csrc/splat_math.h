// pixie_amd/csrc/splat_math.h -- covariance -> 3D Gaussian splat parameters (log-scales, rotation quaternion) for the
// per-frame PLY export (PG/gs_simulation.py:253-288, cov3D_to_log_scales_and_quats).
//
// Register-level math, __host__ __device__ like mpm_math.h (which it does not touch, so that no MPM kernel's code changes):
// the kernels in mpm.hip run it, and tests/host_harness/splat_math_host.cpp checks it on the CPU.
//
// What is computed follows the reference: eigen-decompose the symmetric covariance, sort the eigenvalues descending,
// log_scale = log(sqrt(max(lambda, 1e-12))), R = the matching eigenvectors as columns, made right-handed, quaternion of R (wxyz).
// How it is computed is ours:
//   * cyclic Jacobi in DOUBLE.  The float32 input is converted exactly; the eigenvalues then carry ~1e-16 relative error and
//     the log and quaternion are rounded once to float32 at the end.  float32 Jacobi would leave ~1e-7 lambda_1 in every
//     eigenvalue, and a rounded-twice log-scale (|log| up to ~14 for the clamp) costs up to one more ulp: together that sits at
//     the 1e-6 lambda_1 bar of the tests.  In double the bars hold with margin, and the cost is invisible in a kernel that moves
//     ~100 bytes per Gaussian.
//   * deterministic signs where the reference leaves them to LAPACK: columns 0 and 1 of R have their largest-|.| component
//     positive (the first such component on a tie), column 2 = col0 x col1, so R is right-handed by construction.
//   * quaternion by the branch on the largest of (trace, R00, R11, R22) (scipy's Rotation.from_matrix), normalised, sign
//     chosen so that w >= 0.
// Degenerate spectra (isotropic, two equal eigenvalues) take whatever orthonormal eigenbasis the sweeps reach: any is correct.
// Every array below is indexed with compile-time constants only, so nothing is spilled to scratch.
#pragma once
#include <math.h>

#if defined(__HIPCC__)
#define SPLAT_HD __host__ __device__ __forceinline__
#else
#define SPLAT_HD inline
#endif

namespace pixie {
namespace splat {

constexpr int kMaxSweeps = 12;           // cyclic sweeps; double Jacobi converges quadratically, 4-6 suffice for any input seen
constexpr double kScaleClamp = 1e-12;    // the reference's torch.clamp(evals, min=1e-12)

struct DMat3 {
    double m[9];  // row-major
    SPLAT_HD double& operator()(int r, int c) { return m[3 * r + c]; }
    SPLAT_HD double operator()(int r, int c) const { return m[3 * r + c]; }
};

// One Jacobi rotation annihilating A(P,Q), accumulated into the columns of V.
template <int P, int Q>
SPLAT_HD void rotate(DMat3& A, DMat3& V) {
    const double apq = A(P, Q);
    if (apq == 0.0) return;
    const double app = A(P, P), aqq = A(Q, Q);
    // t = tan(theta) = 2apq / (d + sgn(d) sqrt(d^2 + 4apq^2)), d = aqq - app: the smaller root, |t| <= 1
    const double d = aqq - app;
    const double h = sqrt(d * d + 4.0 * apq * apq);
    const double t = 2.0 * apq / (d + copysign(h, d));
    const double c = 1.0 / sqrt(t * t + 1.0);
    const double s = t * c;
    constexpr int R = 3 - P - Q;
    const double arp = A(R, P), arq = A(R, Q);
    A(P, P) = app - t * apq;
    A(Q, Q) = aqq + t * apq;
    A(P, Q) = 0.0; A(Q, P) = 0.0;
    const double nrp = c * arp - s * arq;
    const double nrq = s * arp + c * arq;
    A(R, P) = nrp; A(P, R) = nrp;
    A(R, Q) = nrq; A(Q, R) = nrq;
    for (int i = 0; i < 3; ++i) {
        const double vp = V(i, P), vq = V(i, Q);
        V(i, P) = c * vp - s * vq;
        V(i, Q) = s * vp + c * vq;
    }
}

// order (lambda_a, column a) before (lambda_b, column b) if lambda_b is larger
template <int A, int B>
SPLAT_HD void sort_pair(double (&l)[3], DMat3& V) {
    if (l[B] > l[A]) {
        const double t = l[A]; l[A] = l[B]; l[B] = t;
        for (int i = 0; i < 3; ++i) { const double v = V(i, A); V(i, A) = V(i, B); V(i, B) = v; }
    }
}

// flip column C of V so that its largest-|.| component (the first on a tie) is positive
template <int C>
SPLAT_HD void fix_sign(DMat3& V) {
    const double a0 = fabs(V(0, C)), a1 = fabs(V(1, C)), a2 = fabs(V(2, C));
    const double big = (a0 >= a1 && a0 >= a2) ? V(0, C) : (a1 >= a2 ? V(1, C) : V(2, C));
    if (big < 0.0)
        for (int i = 0; i < 3; ++i) V(i, C) = -V(i, C);
}

// c6 = (s11, s12, s13, s22, s23, s33), the layout of the frame export's covariance
SPLAT_HD void splat_from_cov(const float c6[6], float log_scale[3], float quat_wxyz[4]) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
    DMat3 A, V;
    A(0, 0) = c6[0]; A(0, 1) = c6[1]; A(0, 2) = c6[2];
    A(1, 0) = c6[1]; A(1, 1) = c6[3]; A(1, 2) = c6[4];
    A(2, 0) = c6[2]; A(2, 1) = c6[4]; A(2, 2) = c6[5];
    for (int i = 0; i < 9; ++i) V.m[i] = (i % 4 == 0) ? 1.0 : 0.0;
    // sweep until the off-diagonal mass is below double resolution against the diagonal (0 <= 0 for the zero matrix;
    // a NaN input never converges and runs kMaxSweeps, giving NaN out)
    for (int sweep = 0; sweep < kMaxSweeps; ++sweep) {
        const double off = A(0, 1) * A(0, 1) + A(0, 2) * A(0, 2) + A(1, 2) * A(1, 2);
        const double dia = A(0, 0) * A(0, 0) + A(1, 1) * A(1, 1) + A(2, 2) * A(2, 2);
        if (off <= 1e-32 * dia) break;
        rotate<0, 1>(A, V);
        rotate<0, 2>(A, V);
        rotate<1, 2>(A, V);
    }
    double l[3] = {A(0, 0), A(1, 1), A(2, 2)};
    sort_pair<0, 1>(l, V);
    sort_pair<1, 2>(l, V);
    sort_pair<0, 1>(l, V);
    for (int i = 0; i < 3; ++i) log_scale[i] = (float)(0.5 * log(fmax(l[i], kScaleClamp)));

    fix_sign<0>(V);
    fix_sign<1>(V);
    // column 2 = col0 x col1: right-handed whatever sign the sweeps left on the third eigenvector
    V(0, 2) = V(1, 0) * V(2, 1) - V(2, 0) * V(1, 1);
    V(1, 2) = V(2, 0) * V(0, 1) - V(0, 0) * V(2, 1);
    V(2, 2) = V(0, 0) * V(1, 1) - V(1, 0) * V(0, 1);

    // quaternion of R = V (scipy Rotation.from_matrix: branch on the largest of trace and the diagonal)
    const double tr = V(0, 0) + V(1, 1) + V(2, 2);
    double w, x, y, z;
    if (tr >= V(0, 0) && tr >= V(1, 1) && tr >= V(2, 2)) {
        w = 1.0 + tr;
        x = V(2, 1) - V(1, 2);
        y = V(0, 2) - V(2, 0);
        z = V(1, 0) - V(0, 1);
    } else if (V(0, 0) >= V(1, 1) && V(0, 0) >= V(2, 2)) {
        x = 1.0 - tr + 2.0 * V(0, 0);
        y = V(1, 0) + V(0, 1);
        z = V(2, 0) + V(0, 2);
        w = V(2, 1) - V(1, 2);
    } else if (V(1, 1) >= V(2, 2)) {
        y = 1.0 - tr + 2.0 * V(1, 1);
        z = V(2, 1) + V(1, 2);
        x = V(0, 1) + V(1, 0);
        w = V(0, 2) - V(2, 0);
    } else {
        z = 1.0 - tr + 2.0 * V(2, 2);
        x = V(0, 2) + V(2, 0);
        y = V(1, 2) + V(2, 1);
        w = V(1, 0) - V(0, 1);
    }
    double inv = 1.0 / sqrt(w * w + x * x + y * y + z * z);
    if (w < 0.0) inv = -inv;
    quat_wxyz[0] = (float)(w * inv);
    quat_wxyz[1] = (float)(x * inv);
    quat_wxyz[2] = (float)(y * inv);
    quat_wxyz[3] = (float)(z * inv);
}

}  // namespace splat
}  // namespace pixie
