// pixie_amd/csrc/ray_sample_math.h -- the per-sample rules of the ray sampling kernels and of the two losses that exist because of
// them (ray_sample.hip), as __host__ __device__ functions, so that tests/host_harness/ray_sample_math_host.cpp runs the same lines on
// the CPU (tests/test_ray_sampling_math.py).  Built with -ffp-contract=off on both sides: every operation below rounds once, in the
// order written, which is the order of the reference's torch expressions.  log, exp and pow are a double evaluation rounded once,
// as ray_render_math.h treats exp; sqrtf and the division are correctly rounded on both sides.
//
//   stratified bin k   lower_k + (upper_k - lower_k) t,   upper_k = (table_k + table_{k+1}) / 2 (table_S for k = S), lower_k likewise
//   euclidean          inv(x s_far + (1 - x) s_near),      s = fn(near | far), fn / inv by spacing kind
//   pdf                w'_i = pow(w_i, anneal) + padding;  sum = sum w'_i;  pad = relu(eps - sum);  pdf_i = (w'_i + pad / S) / (sum + pad)
//   cdf                cdf_0 = 0, cdf_{i+1} = min(1, running sum of pdf), made non-decreasing by a running maximum
//   new bin            b0 + clip(nan_to_num((u - c0) / (c1 - c0), 0), 0, 1) (b1 - b0),  (c0, c1, b0, b1) at searchsorted(cdf, u, right) - 1 | + 0
//   interlevel         clip(w - w_outer, 0)^2 / (w + 1e-7),  w_outer = sum_{j = lo .. hi} w_env_j, added in index order
//   distortion         sum_i w_i sum_j w_j |u_i - u_j| + (sum_i w_i^2 (t_{i+1} - t_i)) / 3,   u_i = (t_{i+1} + t_i) / 2
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RS_HD __host__ __device__ inline
#else
#define RS_HD inline
#endif

namespace pixie {
namespace rs {

constexpr int kMaxSamples = 1024;          // existing and produced samples per ray: one wave per ray, edges staged in LDS
constexpr int kMaxLevels = 8;              // proposal levels of one interlevel call
constexpr int64_t kMaxRays = (int64_t)1 << 24;
// kForeign: the caller's own spacing_to_euclidean_fn, applied in torch: the kernel stops at the spacing bins
enum Spacing { kForeign = -1, kUniform = 0, kLinDisp = 1, kSqrt = 2, kLog = 3, kPiecewise = 4 };

RS_HD int samples_per_lane(int n) { return (n + 63) / 64; }

RS_HD float log_of(float x) { return (float)log((double)x); }
RS_HD float exp_of(float x) { return (float)exp((double)x); }
RS_HD float pow_of(float x, float e) { return (float)pow((double)x, (double)e); }

// ---- spacing functions (ray_samplers.py: the five SpacedSampler subclasses) ------------------------------------------------------
RS_HD float spacing_fn(int kind, float x) {
    switch (kind) {
        case kLinDisp: return 1.0f / x;
        case kSqrt: return sqrtf(x);
        case kLog: return log_of(x);
        case kPiecewise: return x < 1.0f ? x / 2.0f : 1.0f - 1.0f / (2.0f * x);
        default: return x;
    }
}
RS_HD float spacing_fn_inv(int kind, float s) {
    switch (kind) {
        case kLinDisp: return 1.0f / s;
        case kSqrt: return s * s;
        case kLog: return exp_of(s);
        case kPiecewise: return s < 0.5f ? 2.0f * s : 1.0f / (2.0f - 2.0f * s);
        default: return s;
    }
}
RS_HD float to_euclidean(int kind, float x, float s_near, float s_far) { return spacing_fn_inv(kind, x * s_far + (1.0f - x) * s_near); }

// ---- stratified bins of the spaced samplers --------------------------------------------------------------------------------------
RS_HD float bin_center(float lo, float hi) { return (hi + lo) / 2.0f; }
// table: the S + 1 values of linspace(0, 1, S + 1); t the jitter of bin k
RS_HD float stratified_bin(const float* table, int k, int n_samples, float t) {
    const float upper = k < n_samples ? bin_center(table[k], table[k + 1]) : table[n_samples];
    const float lower = k > 0 ? bin_center(table[k - 1], table[k]) : table[0];
    return lower + (upper - lower) * t;
}

// ---- what get_ray_samples and Frustums.get_positions derive from two euclidean edges ----------------------------------------------
RS_HD float delta_of(float start, float end) { return end - start; }
RS_HD float position(float origin, float direction, float start, float end) { return origin + direction * (start + end) / 2.0f; }

// ---- PDFSampler -------------------------------------------------------------------------------------------------------------------
RS_HD float histogram_weight(float w, float anneal, float padding) { return (anneal == 1.0f ? w : pow_of(w, anneal)) + padding; }
RS_HD float empty_padding(float sum, float eps) {                  // relu(eps - sum): a NaN stays a NaN
    const float d = eps - sum;
    return d < 0.0f ? 0.0f : d;
}
RS_HD float pdf_of(float w, float share, float total) { return (w + share) / total; }
RS_HD float cdf_clamp(float running) { return running > 1.0f ? 1.0f : running; }          // min(1, .) of finite values
RS_HD float running_max(float so_far, float v) { return v > so_far ? v : so_far; }        // a NaN never replaces a number

// torch.searchsorted on one sorted row: the number of entries <= v (right) or < v (left)
RS_HD int count_le(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (v < a[mid]) hi = mid; else lo = mid + 1;
    }
    return lo;
}
RS_HD int count_lt(const float* a, int n, float v) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (a[mid] < v) lo = mid + 1; else hi = mid;
    }
    return lo;
}
RS_HD int clamp_index(int i, int lo, int hi) { return i < lo ? lo : i > hi ? hi : i; }

// clip(nan_to_num(q, nan = 0), 0, 1): NaN -> 0, +Inf -> FLT_MAX -> 1, -Inf -> -FLT_MAX -> 0
RS_HD float unit_clip(float q) {
    if (q != q) return 0.0f;
    return q < 0.0f ? 0.0f : q > 1.0f ? 1.0f : q;
}
RS_HD float cdf_interp(float u, float c0, float c1, float b0, float b1) {
    const float t = unit_clip((u - c0) / (c1 - c0));
    return b0 + t * (b1 - b0);
}

// ---- interlevel loss (losses.py: outer, lossfun_outer) ------------------------------------------------------------------------------
constexpr float kOuterEps = 1e-7f;
// edges: the S_env + 1 proposal edges; the fine interval [c0, c1] is covered by the proposal intervals lo .. hi
RS_HD int outer_lo(const float* edges, int n_env, float c0) { return clamp_index(count_le(edges, n_env, c0) - 1, 0, n_env - 1); }
RS_HD int outer_hi(const float* edges, int n_env, float c1) { return clamp_index(count_le(edges + 1, n_env, c1), 0, n_env - 1); }
// the enclosed weight, summed directly in index order: the reference's difference of two running sums loses what a float32 running
// sum near 1 cannot hold (an ulp of 1 is 6e-8, and the loss divides by w + 1e-7)
RS_HD float outer_sum(const float* w_env, int lo, int hi) {
    float s = 0.0f;
    for (int j = lo; j <= hi; ++j) s = s + w_env[j];
    return s;
}
RS_HD float outer_excess(float w, float w_outer) {
    const float d = w - w_outer;
    return d < 0.0f ? 0.0f : d;                                    // clip(., min = 0): a NaN stays a NaN
}
RS_HD float outer_term(float w, float w_outer) {
    const float d = outer_excess(w, w_outer);
    return d * d / (w + kOuterEps);
}
// d term / d w_outer, times the upstream scale
RS_HD float outer_term_grad(float w, float w_outer, float scale) { return -(2.0f * outer_excess(w, w_outer)) / (w + kOuterEps) * scale; }

// ---- distortion loss (losses.py: lossfun_distortion) ---------------------------------------------------------------------------------
RS_HD float interval_mid(float t0, float t1) { return (t1 + t0) / 2.0f; }
RS_HD float distortion_pair(float w_j, float u_i, float u_j) { return w_j * fabsf(u_i - u_j); }
RS_HD float distortion_intra(float w, float t0, float t1) { return w * w * (t1 - t0); }
RS_HD float distortion_ray(float inter, float intra) { return inter + intra / 3.0f; }
RS_HD float distortion_grad(float inner, float w, float t0, float t1, float scale) {
    return (2.0f * inner + 2.0f * w * (t1 - t0) / 3.0f) * scale;
}

}  // namespace rs
}  // namespace pixie
