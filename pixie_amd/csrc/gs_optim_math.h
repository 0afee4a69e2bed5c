// pixie_amd/csrc/gs_optim_math.h -- per-element arithmetic of the 3DGS training step after the backward pass: the Adam update of
// torch.optim.Adam's default path, the densification statistics of train.py:114-116 and the decisions and new values of
// scene/gaussian_model.py:densify_and_prune (:353-405).
//
// Register-level math, __host__ __device__ like knn_math.h and ingest_math.h: the kernels in gs_optim.hip run it and a host
// compiler can build it for CPU checks.  Everything is float32 and gs_optim.hip is built with -ffp-contract=off, so the order of
// operations written here is the order the device rounds in.
//   adam_element()        m = lerp(m, g, 1 - beta1); v = v beta2 + (1 - beta2) g g; p -= step_size m / (sqrt(v) / bc2_sqrt + eps)
//   stats_norm2()         sqrt(gx gx + gy gy)
//   mean_grad()           accum / denom with NaN -> 0
//   max_scale()           max(exp(s0), exp(s1), exp(s2))
//   sigmoid()             1 / (1 + exp(-x))
//   classify()            clone / split and the final prune of the row, its clone and its two children -> which rows it leaves
//   split_scaling()       log(exp(s) / 1.6)
//   split_position()      R(q / |q|) (exp(s) * z) + xyz, R as utils/general_utils.py:build_rotation writes it
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define GSO_HD __host__ __device__ __forceinline__
#else
#define GSO_HD inline
#endif

namespace pixie {
namespace gso {

constexpr int kMaxGroups = 8;
constexpr float kSplitShrink = 1.6f;      // 0.8 * N with N = 2 children per split Gaussian

// One element of torch.optim.Adam (no weight decay, no amsgrad, not maximize).  w1 = float(1 - beta1), w2 = float(1 - beta2):
// the scalars torch hands its kernels.  lerp with a weight below 0.5 is start + weight * (end - start), as ATen writes it; the
// other branch is there for a beta1 below 0.5.
GSO_HD void adam_element(float& p, float g, float& m, float& v, float w1, float beta2, float w2, float eps, float step_size,
                         float bc2_sqrt) {
    const float diff = g - m;
    m = w1 < 0.5f ? m + w1 * diff : g - diff * (1.0f - w1);
    v = v * beta2 + (w2 * g) * g;
    const float denom = sqrtf(v) / bc2_sqrt + eps;
    p = p + (-step_size) * (m / denom);
}

GSO_HD float stats_norm2(float gx, float gy) { return sqrtf(gx * gx + gy * gy); }

GSO_HD float mean_grad(float accum, float denom) {
    const float g = accum / denom;
    return g != g ? 0.0f : g;
}

GSO_HD float max_scale(const float s[3]) { return fmaxf(fmaxf(expf(s[0]), expf(s[1])), expf(s[2])); }

GSO_HD float sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }

GSO_HD void split_scaling(const float s[3], float out[3]) {
    for (int k = 0; k < 3; ++k) out[k] = logf(expf(s[k]) / kSplitShrink);
}

// bit 0: the original row stays (not split, not pruned); bit 1: a clone of it stays; bit 2: its two split children stay (both or
// neither: they share scaling and opacity); bit 3: it is split; bit 4: it is cloned (the clone kept or not).
enum { kKeepSelf = 1, kKeepClone = 2, kKeepChildren = 4, kIsSplit = 8, kIsClone = 16 };

// dense_thr = float(percent_dense * extent), world_thr = float(0.1 * extent): the Python scalars the reference compares with.
GSO_HD int classify(float accum, float denom, const float s[3], float opacity, float max_grad, float dense_thr, float min_opacity,
                    int has_world_thr, float world_thr) {
    const float g = mean_grad(accum, denom);
    const float smax = max_scale(s);
    const bool selected = g >= max_grad;
    const bool clone = selected && smax <= dense_thr;
    const bool split = selected && smax > dense_thr;
    const bool faint = sigmoid(opacity) < min_opacity;
    const bool prune_self = faint || (has_world_thr && smax > world_thr);
    int flags = 0;
    if (!split && !prune_self) flags |= kKeepSelf;
    if (clone) flags |= kIsClone;
    if (clone && !prune_self) flags |= kKeepClone;
    if (split) {
        flags |= kIsSplit;
        float ns[3];
        split_scaling(s, ns);
        const bool prune_child = faint || (has_world_thr && max_scale(ns) > world_thr);
        if (!prune_child) flags |= kKeepChildren;
    }
    return flags;
}

GSO_HD void split_position(const float xyz[3], const float s[3], const float r[4], const float z[3], float out[3]) {
    const float norm = sqrtf(r[0] * r[0] + r[1] * r[1] + r[2] * r[2] + r[3] * r[3]);
    const float qr = r[0] / norm, qx = r[1] / norm, qy = r[2] / norm, qz = r[3] / norm;
    const float R[3][3] = {{1.0f - 2.0f * (qy * qy + qz * qz), 2.0f * (qx * qy - qr * qz), 2.0f * (qx * qz + qr * qy)},
                           {2.0f * (qx * qy + qr * qz), 1.0f - 2.0f * (qx * qx + qz * qz), 2.0f * (qy * qz - qr * qx)},
                           {2.0f * (qx * qz - qr * qy), 2.0f * (qy * qz + qr * qx), 1.0f - 2.0f * (qx * qx + qy * qy)}};
    const float smp[3] = {expf(s[0]) * z[0], expf(s[1]) * z[1], expf(s[2]) * z[2]};
    for (int k = 0; k < 3; ++k) out[k] = ((R[k][0] * smp[0] + R[k][1] * smp[1]) + R[k][2] * smp[2]) + xyz[k];
}

}  // namespace gso
}  // namespace pixie
