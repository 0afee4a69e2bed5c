// pixie_amd/csrc/ray_render_math.h -- the per-sample rules of the ray compositing kernels (ray_render.hip), as __host__ __device__
// functions, so that tests/host_harness/ray_render_math_host.cpp runs the same lines on the CPU against a float64 restatement of
// the reference's get_weights and renderers (tests/test_ray_render_math.py).  Built with -ffp-contract=off on both sides: every
// operation below rounds once, in the order written.  expf(-x) is evaluated as float(exp(-double(x))) on both sides: a float32 exp good
// to one ulp errs with a bias of a fraction of an ulp near 1, which alpha = 1 - expf(-x) amplifies at small x and a 1000-sample sum
// then adds up (measured on the device: accumulation off by 8e-6 at S = 1000 against 1e-6 for a correctly rounded expf); the double
// exp rounded once is correctly rounded but for a vanishing share of arguments, so g++ and the device agree to the last bit nearly always.
//
//   x_i     = delta_i * sigma_i                          optical depth of sample i
//   alpha_i = 1 - expf(-x_i)
//   w_i     = nan_to_num(alpha_i * expf(-P_i)),          P_i = sum_{j < i} x_j  (the last sample's x enters no prefix)
//   m_i     = (start_i + end_i) / 2
//   D       = N / (A + 1e-10f),   N = sum w_i m_i,  A = sum w_i;    dD/dN = 1 / (A + 1e-10f),  dD/dA = -N / (A + 1e-10f)^2
//   median  = m_j, j the first index whose inclusive running sum of w reaches 0.5, S - 1 if none does
//   dL/dx_k = g_k expf(-x_k) expf(-P_k) - sum_{i > k} g_i w_i,   g_i = dL/dw_i, set to 0 where nan_to_num replaced the weight
#pragma once
#include <float.h>
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define RR_HD __host__ __device__ inline
#else
#define RR_HD inline
#endif

namespace pixie {
namespace rr {

constexpr int kMaxSamples = 1024;          // ray kernels: one wave per ray, 64 lanes of at most 16 consecutive samples
constexpr int kMaxFeatureSamples = 256;    // feature kernels
constexpr int kMaxChannels = 2048;
constexpr int kChunk = 256;                // channels per wave in the feature kernels: 64 lanes of one float4
constexpr int64_t kMaxRays = (int64_t)1 << 24;
enum Background { kBgNone = 0, kBgConstant = 1, kBgLastSample = 2 };

RR_HD int samples_per_lane(int n_samples) { return (n_samples + 63) / 64; }
RR_HD int chunks_of(int n_channels) { return (n_channels + kChunk - 1) / kChunk; }

RR_HD float exp_neg(float x) { return (float)exp(-(double)x); }           // expf(-x), correctly rounded
RR_HD float optical_depth(float delta, float sigma) { return delta * sigma; }
RR_HD float alpha_of(float x) { return 1.0f - exp_neg(x); }
RR_HD float transmittance(float prefix) { return exp_neg(prefix); }
RR_HD float raw_weight(float alpha, float t) { return alpha * t; }

// torch.nan_to_num's defaults: NaN -> 0, +Inf -> FLT_MAX, -Inf -> -FLT_MAX
RR_HD bool replaced(float w) { return !(fabsf(w) <= FLT_MAX); }
RR_HD float nan_to_num(float w) {
    if (w != w) return 0.0f;
    if (w > FLT_MAX) return FLT_MAX;
    if (w < -FLT_MAX) return -FLT_MAX;
    return w;
}
RR_HD float weight(float x, float prefix) { return nan_to_num(raw_weight(alpha_of(x), transmittance(prefix))); }

RR_HD float midpoint(float start, float end) { return (start + end) / 2.0f; }

RR_HD float expected_depth(float n, float a) { return n / (a + 1e-10f); }
RR_HD float d_depth_d_n(float a) { return 1.0f / (a + 1e-10f); }
RR_HD float d_depth_d_a(float n, float a) {
    const float d = a + 1e-10f;
    return -n / (d * d);
}
// dD/dw_i = m_i dD/dN + dD/dA
RR_HD float d_depth_d_weight(float mid, float dn, float da) { return mid * dn + da; }

// the median index: the first i with median_reached(inclusive running sum), else the last sample
RR_HD bool median_reached(float cumulative) { return cumulative >= 0.5f; }
RR_HD int median_index(int first_reached, int n_samples) { return first_reached < n_samples ? first_reached : n_samples - 1; }

// the first term of dL/dx_k; a replaced weight passes no gradient (0, not 0 * NaN)
RR_HD float d_x_own(float g, float x, float prefix, bool was_replaced) {
    return was_replaced ? 0.0f : g * exp_neg(x) * transmittance(prefix);
}

}  // namespace rr
}  // namespace pixie
