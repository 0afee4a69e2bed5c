// pixie_amd/csrc/knn_math.h -- arithmetic of distCUDA2 (simple-knn): the mean squared distance of a point to its three nearest
// other points, as gaussian-splatting/scene/gaussian_model.py:create_from_pcd initialises every Gaussian's scale from.
//
// Register-level math, __host__ __device__ like raster_math.h and ingest_math.h: the kernels in knn.hip run it and
// tests/host_harness/knn_math_host.cpp checks it on the CPU.  Everything is float32 and both sides are built with
// -ffp-contract=off, so the device result is bit-equal to a float32 brute force that uses the same expression order:
//   morton_axis() / morton3()   30-bit Morton code of a point inside the cloud's bounding box; an axis of zero extent maps to 0
//   dist2()                     ((dx dx + dy dy) + dz dz), d = q - p
//   box_point_dist2()           the same expression on the per-axis distances of a point to a box
//   box_box_dist2()             the same expression on the per-axis gaps between two boxes
//   insert3()                   keeps the three smallest values seen, ascending
//   mean3()                     ((b0 + b1) + b2) / 3
//
// Why pruning with the float32 bounds is exact.  For a point q inside a box [lo, hi] and any p, the real number |q.x - p.x| is at
// least the real per-axis distance of p to the box (lo.x - p.x, p.x - hi.x or 0).  Both differences are rounded to float32 by the
// same monotone rounding, so the rounded |q.x - p.x| is at least the rounded axis distance; negation is exact, so the sign of the
// difference does not matter.  Squares, and sums taken in the same order, of non-negative floats are monotone in every operand as
// well.  Hence box_point_dist2(lo, hi, p) <= dist2(p, q) holds for the float32 VALUES, not merely up to rounding, and a box whose
// bound exceeds a point's current third-best distance cannot hold a closer point.  The same argument, with p ranging over a second
// box, covers box_box_dist2().  Input must be finite: a NaN coordinate compares false everywhere, so the affected points get
// unspecified values (loops are counted, nothing hangs or leaves its bounds).
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define KNN_HD __host__ __device__ __forceinline__
#else
#define KNN_HD inline
#endif

namespace pixie {
namespace knn {

constexpr int kGroup = 64;               // consecutive Morton-sorted points per box: one wave, one point per lane
constexpr int64_t kMaxPoints = 1 << 24;

// 10 bits -> every third bit of 30
KNN_HD uint32_t spread10(uint32_t x) {
    x = (x | (x << 16)) & 0x030000FFu;
    x = (x | (x << 8)) & 0x0300F00Fu;
    x = (x | (x << 4)) & 0x030C30C3u;
    x = (x | (x << 2)) & 0x09249249u;
    return x;
}

// 10-bit cell of v in [lo, hi]; 0 when the axis has no extent (no division by zero) or v is not a number
KNN_HD uint32_t morton_axis(float v, float lo, float hi) {
    const float extent = hi - lo;
    if (!(extent > 0.0f)) return 0u;
    const float t = ((v - lo) / extent) * 1023.0f;
    if (!(t > 0.0f)) return 0u;
    return t >= 1023.0f ? 1023u : (uint32_t)t;
}

KNN_HD uint32_t morton3(const float* p, const float* lo, const float* hi) {
    return spread10(morton_axis(p[0], lo[0], hi[0])) | (spread10(morton_axis(p[1], lo[1], hi[1])) << 1) |
           (spread10(morton_axis(p[2], lo[2], hi[2])) << 2);
}

KNN_HD float sum_sq(float dx, float dy, float dz) { return (dx * dx + dy * dy) + dz * dz; }

KNN_HD float dist2(float px, float py, float pz, float qx, float qy, float qz) { return sum_sq(qx - px, qy - py, qz - pz); }

// distance of v to the interval [lo, hi] along one axis
KNN_HD float axis_gap(float lo, float hi, float v) { return v < lo ? lo - v : (v > hi ? v - hi : 0.0f); }

KNN_HD float box_point_dist2(const float* lo, const float* hi, float px, float py, float pz) {
    return sum_sq(axis_gap(lo[0], hi[0], px), axis_gap(lo[1], hi[1], py), axis_gap(lo[2], hi[2], pz));
}

// gap between the intervals [alo, ahi] and [blo, bhi] along one axis
KNN_HD float axis_gap2(float alo, float ahi, float blo, float bhi) { return blo > ahi ? blo - ahi : (alo > bhi ? alo - bhi : 0.0f); }

KNN_HD float box_box_dist2(const float* alo, const float* ahi, const float* blo, const float* bhi) {
    return sum_sq(axis_gap2(alo[0], ahi[0], blo[0], bhi[0]), axis_gap2(alo[1], ahi[1], blo[1], bhi[1]),
                  axis_gap2(alo[2], ahi[2], blo[2], bhi[2]));
}

// b0 <= b1 <= b2 are the three smallest values so far; d joins them if it is smaller than b2.  fminf / fmaxf drop a NaN.
KNN_HD void insert3(float d, float& b0, float& b1, float& b2) {
    const float n2 = fminf(b2, fmaxf(b1, d)), n1 = fminf(b1, fmaxf(b0, d)), n0 = fminf(b0, d);
    b0 = n0; b1 = n1; b2 = n2;
}

// a missing neighbour is FLT_MAX, as in simple-knn: one or two points give +inf (the sum overflows), three give FLT_MAX / 3
KNN_HD float mean3(float b0, float b1, float b2) { return ((b0 + b1) + b2) / 3.0f; }

}  // namespace knn
}  // namespace pixie
