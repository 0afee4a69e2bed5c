// tests/host_harness/ray_sample_math_host.cpp -- pixie_amd/csrc/ray_sample_math.h built for the host (g++ -ffp-contract=off), for
// tests/test_ray_sampling_math.py: the per-sample rules one by one, and one ray walked with them in float32, sums front to back.
#include "../../pixie_amd/csrc/ray_sample_math.h"

using namespace pixie::rs;

extern "C" {

float hh_rs_spacing_fn(int kind, float x) { return spacing_fn(kind, x); }
float hh_rs_to_euclidean(int kind, float x, float s_near, float s_far) { return to_euclidean(kind, x, s_near, s_far); }
float hh_rs_delta(float start, float end) { return delta_of(start, end); }
float hh_rs_position(float o, float d, float start, float end) { return position(o, d, start, end); }
float hh_rs_cdf_interp(float u, float c0, float c1, float b0, float b1) { return cdf_interp(u, c0, c1, b0, b1); }
float hh_rs_histogram_weight(float w, float anneal, float padding) { return histogram_weight(w, anneal, padding); }
int hh_rs_count_le(const float* a, int n, float v) { return count_le(a, n, v); }
int hh_rs_count_lt(const float* a, int n, float v) { return count_lt(a, n, v); }
int hh_rs_limit(int which) { return which == 0 ? kMaxSamples : kMaxLevels; }
int hh_rs_samples_per_lane(int n) { return samples_per_lane(n); }

// the S + 1 stratified bins of one ray; stride 1: one jitter for the ray, else one per bin
void hh_rs_stratified_row(const float* table, int n_samples, const float* jitter, int stride, float* out) {
    for (int k = 0; k <= n_samples; ++k) out[k] = stratified_bin(table, k, n_samples, jitter[stride == 1 ? 0 : k]);
}

// one ray of the pdf sampler: cdf (S + 1) and the n_u new bins, merged with the existing edges into out when include_original
void hh_rs_pdf_row(const float* existing, const float* w, int S, const float* u, int n_u, float padding, float eps, float anneal,
                   int include_original, float* cdf, float* out) {
    float h[kMaxSamples], fresh[kMaxSamples + 1];
    float sum = 0.0f;
    for (int i = 0; i < S; ++i) {
        h[i] = histogram_weight(w[i], anneal, padding);
        sum = sum + h[i];
    }
    const float pad = empty_padding(sum, eps);
    const float share = pad / (float)S, total = sum + pad;
    float running = 0.0f, top = 0.0f;
    cdf[0] = 0.0f;
    for (int i = 0; i < S; ++i) {
        running = running + pdf_of(h[i], share, total);
        top = running_max(top, cdf_clamp(running));
        cdf[i + 1] = top;
    }
    for (int k = 0; k < n_u; ++k) {
        const int inds = count_le(cdf, S + 1, u[k]);
        const int below = clamp_index(inds - 1, 0, S), above = clamp_index(inds, 0, S);
        fresh[k] = cdf_interp(u[k], cdf[below], cdf[above], existing[below], existing[above]);
    }
    if (!include_original) {
        for (int k = 0; k < n_u; ++k) out[k] = fresh[k];
        return;
    }
    for (int k = 0; k < n_u; ++k) out[k + count_le(existing, S + 1, fresh[k])] = fresh[k];
    for (int i = 0; i <= S; ++i) out[i + count_lt(fresh, n_u, existing[i])] = existing[i];
}

// one ray of lossfun_outer: the S terms, and d (sum_i up_i term_i) / d w_env gathered in index order
void hh_rs_outer_row(const float* c, const float* w, int S, const float* c_env, const float* w_env, int n_env, const float* up, float* terms,
                     float* d_w_env) {
    float g[kMaxSamples];
    int lo[kMaxSamples], hi[kMaxSamples];
    for (int i = 0; i < S; ++i) {
        lo[i] = outer_lo(c_env, n_env, c[i]), hi[i] = outer_hi(c_env, n_env, c[i + 1]);
        const float w_outer = outer_sum(w_env, lo[i], hi[i]);
        terms[i] = outer_term(w[i], w_outer);
        g[i] = outer_term_grad(w[i], w_outer, up[i]);
    }
    for (int j = 0; j < n_env; ++j) {
        float acc = 0.0f;
        for (int i = 0; i < S; ++i)
            if (lo[i] <= j && j <= hi[i]) acc = acc + g[i];
        d_w_env[j] = acc;
    }
}

// one ray of lossfun_distortion and its gradient times `scale`
float hh_rs_distortion_row(const float* t, const float* w, int S, float scale, float* d_w) {
    float u[kMaxSamples];
    for (int i = 0; i < S; ++i) u[i] = interval_mid(t[i], t[i + 1]);
    float inter = 0.0f, intra = 0.0f;
    for (int i = 0; i < S; ++i) {
        float inner = 0.0f;
        for (int j = 0; j < S; ++j) inner = inner + distortion_pair(w[j], u[i], u[j]);
        inter = inter + w[i] * inner;
        intra = intra + distortion_intra(w[i], t[i], t[i + 1]);
        d_w[i] = distortion_grad(inner, w[i], t[i], t[i + 1], scale);
    }
    return distortion_ray(inter, intra);
}

}  // extern "C"
