// tests/host_harness/ray_render_math_host.cpp -- pixie_amd/csrc/ray_render_math.h built for the host (g++ -ffp-contract=off), for
// tests/test_ray_render_math.py: the per-sample rules one by one, and one ray walked front to back with them, in float32.
#include "../../pixie_amd/csrc/ray_render_math.h"

using namespace pixie::rr;

extern "C" {

float hh_rr_alpha(float x) { return alpha_of(x); }
float hh_rr_weight(float x, float prefix) { return weight(x, prefix); }
float hh_rr_nan_to_num(float w) { return nan_to_num(w); }
int hh_rr_replaced(float w) { return replaced(w) ? 1 : 0; }
float hh_rr_midpoint(float s, float e) { return midpoint(s, e); }
float hh_rr_expected_depth(float n, float a) { return expected_depth(n, a); }
float hh_rr_d_depth_d_n(float a) { return d_depth_d_n(a); }
float hh_rr_d_depth_d_a(float n, float a) { return d_depth_d_a(n, a); }
float hh_rr_d_depth_d_weight(float mid, float dn, float da) { return d_depth_d_weight(mid, dn, da); }
int hh_rr_median_index(const float* w, int n) {
    float cumulative = 0.0f;
    int first = n;
    for (int i = 0; i < n; ++i) {
        cumulative = cumulative + w[i];
        if (first == n && median_reached(cumulative)) first = i;
    }
    return median_index(first, n);
}
int hh_rr_samples_per_lane(int s) { return samples_per_lane(s); }
int hh_rr_chunks(int c) { return chunks_of(c); }
int hh_rr_limit(int which) { return which == 0 ? kMaxSamples : which == 1 ? kMaxFeatureSamples : which == 2 ? kMaxChannels : kChunk; }

// one ray, front to back: weights, accumulation, unclipped expected depth
void hh_rr_ray_forward(const float* delta, const float* sigma, const float* start, const float* end, int n, float* w, float* acc, float* depth) {
    float prefix = 0.0f, a = 0.0f, num = 0.0f;
    for (int i = 0; i < n; ++i) {
        const float x = optical_depth(delta[i], sigma[i]);
        w[i] = weight(x, prefix);
        prefix = prefix + x;
        a = a + w[i];
        num = num + w[i] * midpoint(start[i], end[i]);
    }
    *acc = a;
    *depth = expected_depth(num, a);
}

// d_density from g = dL/dw: the masked own term minus the suffix sum of g w, times delta
void hh_rr_ray_backward(const float* delta, const float* sigma, const float* g, int n, float* d_sigma) {
    float prefix = 0.0f;
    float own[kMaxSamples], gw[kMaxSamples];
    for (int i = 0; i < n; ++i) {
        const float x = optical_depth(delta[i], sigma[i]);
        const bool masked = replaced(raw_weight(alpha_of(x), transmittance(prefix)));
        const float gi = masked ? 0.0f : g[i];
        own[i] = d_x_own(gi, x, prefix, masked);
        gw[i] = masked ? 0.0f : gi * weight(x, prefix);
        prefix = prefix + x;
    }
    float after = 0.0f;
    for (int i = n - 1; i >= 0; --i) {
        d_sigma[i] = delta[i] * (own[i] - after);
        after = after + gw[i];
    }
}

}  // extern "C"
