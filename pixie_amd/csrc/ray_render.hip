// pixie_amd/csrc/ray_render.hip -- differentiable ray compositing: get_weights, the rgb / accumulation / depth renderers and the
// C-wide feature sum of a NeRF training step, forward and backward (include/pixie_hip.h).
//
// Four kernels.  The ray kernels run one wave per ray: lane l owns the q = ceil(S / 64) consecutive samples from l q, sums them
// sequentially and the lanes' sums are scanned or reduced over the wave in a fixed order.  The feature kernels run one wave per
// (ray, chunk of 256 channels), four channels (16 bytes) per lane, and walk the samples in ascending order: one accumulator chain
// per channel, so no sum depends on the launch geometry.  No floating-point atomics; every sum has one order.
// Built with -ffp-contract=off: the per-sample arithmetic is ray_render_math.h as g++ rounds it (its exp goes through double).
#include "../../include/pixie_hip.h"
#include "common.h"
#include "ray_render_math.h"
#include "wave_order.h"   // wave_sum, wave_min, wave_exclusive_prefix / _suffix: fixed order

namespace pixie {
namespace {

constexpr int kWavesPerBlock = 4;
constexpr int kBlock = 64 * kWavesPerBlock;

struct RayParams {
    const float* densities;     // (R, S) or nullptr: "weights given"
    const float* deltas;        // (R, S)
    const float* weights;       // (R, S): given, or (backward) the forward's output
    const float* starts;        // (R, S) or nullptr
    const float* ends;
    const float* rgb;           // (R, S, 3) or nullptr
    int64_t n_rays;
    int n_samples, per_lane, chunks, background;
    float bg[3];
};

struct RaySums {
    float a, n, c[3];
};

// A = sum w, N = sum w m, colour sums: the lane's samples in ascending order, then the wave.  Forward and backward both call
// this on the same array, so the backward sees the forward's bits.
__device__ inline RaySums ray_sums(const RayParams& p, const float* w, int64_t base, int i0, int i1, bool want_n, bool want_rgb) {
    RaySums s = {0.0f, 0.0f, {0.0f, 0.0f, 0.0f}};
    for (int i = i0; i < i1; ++i) {
        const float wi = w[base + i];
        s.a = s.a + wi;
        if (want_n) s.n = s.n + wi * rr::midpoint(p.starts[base + i], p.ends[base + i]);
        if (want_rgb) {
            const float* c = p.rgb + (base + i) * 3;
            s.c[0] = s.c[0] + wi * c[0];
            s.c[1] = s.c[1] + wi * c[1];
            s.c[2] = s.c[2] + wi * c[2];
        }
    }
    s.a = wave_sum(s.a);
    if (want_n) s.n = wave_sum(s.n);
    if (want_rgb) {
        s.c[0] = wave_sum(s.c[0]);
        s.c[1] = wave_sum(s.c[1]);
        s.c[2] = wave_sum(s.c[2]);
    }
    return s;
}

__device__ inline void background_of(const RayParams& p, int64_t base, float bg[3]) {
    if (p.background == rr::kBgLastSample) {
        const float* c = p.rgb + (base + p.n_samples - 1) * 3;
        bg[0] = c[0], bg[1] = c[1], bg[2] = c[2];
    } else {
        bg[0] = p.bg[0], bg[1] = p.bg[1], bg[2] = p.bg[2];
    }
}

// ---- ray forward ------------------------------------------------------------------------------------------------------------
struct RayForwardOut {
    float* weights;          // (R, S), density mode only
    float* accumulation;     // (R)
    float* expected_depth;   // (R), unclipped
    float* median_depth;     // (R)
    float* rgb;              // (R, 3)
};

__global__ __launch_bounds__(kBlock) void ray_forward_kernel(RayParams p, RayForwardOut o) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= p.n_rays) return;                                   // whole waves leave; the kernel has no barrier
    const int S = p.n_samples;
    const int i0 = min(lane * p.per_lane, S), i1 = min(i0 + p.per_lane, S);
    const int64_t base = ray * S;
    const float* w = p.weights;
    if (p.densities) {
        float local = 0.0f;
        for (int i = i0; i < i1; ++i) local = local + rr::optical_depth(p.deltas[base + i], p.densities[base + i]);
        float prefix = wave_exclusive_prefix(local, lane);
        for (int i = i0; i < i1; ++i) {
            const float x = rr::optical_depth(p.deltas[base + i], p.densities[base + i]);
            o.weights[base + i] = rr::weight(x, prefix);
            prefix = prefix + x;
        }
        w = o.weights;                                             // a lane reads back only what it wrote itself
    }
    const bool want_n = o.expected_depth != nullptr, want_rgb = o.rgb != nullptr;
    if (!(o.accumulation || want_n || want_rgb || o.median_depth)) return;
    const RaySums s = ray_sums(p, w, base, i0, i1, want_n, want_rgb);
    if (o.median_depth) {
        float local = 0.0f;
        for (int i = i0; i < i1; ++i) local = local + w[base + i];
        float cumulative = wave_exclusive_prefix(local, lane);
        int first = S;
        for (int i = i0; i < i1; ++i) {
            cumulative = cumulative + w[base + i];
            if (first == S && rr::median_reached(cumulative)) first = i;
        }
        const int j = rr::median_index(wave_min(first), S);
        if (lane == 0) o.median_depth[ray] = rr::midpoint(p.starts[base + j], p.ends[base + j]);
    }
    if (lane != 0) return;
    if (o.accumulation) o.accumulation[ray] = s.a;
    if (want_n) o.expected_depth[ray] = rr::expected_depth(s.n, s.a);
    if (want_rgb) {
        if (p.background == rr::kBgNone) {
            o.rgb[ray * 3 + 0] = s.c[0], o.rgb[ray * 3 + 1] = s.c[1], o.rgb[ray * 3 + 2] = s.c[2];
        } else {
            float bg[3];
            background_of(p, base, bg);
            const float rest = 1.0f - s.a;
            for (int c = 0; c < 3; ++c) o.rgb[ray * 3 + c] = s.c[c] + bg[c] * rest;
        }
    }
}

// ---- ray backward -----------------------------------------------------------------------------------------------------------
struct RayBackwardArgs {
    const float* up_weights;        // (R, S)    dL/d weights output (density mode)
    const float* up_accumulation;   // (R)
    const float* up_depth;          // (R)       dL/d unclipped expected depth
    const float* up_rgb;            // (R, 3)
    const float* partial;           // (R, chunks, S) from the feature backward, or nullptr
    float* d_densities;             // (R, S) density mode
    float* d_weights;               // (R, S) weights mode
    float* d_rgb;                   // (R, S, 3)
};

// Q = samples per lane: the lane's g w and own terms stay in registers between the ascending and the descending walk
template <int Q>
__global__ __launch_bounds__(kBlock) void ray_backward_kernel(RayParams p, RayBackwardArgs b) {
    const int lane = threadIdx.x & 63;
    const int64_t ray = (int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6);
    if (ray >= p.n_rays) return;
    const int S = p.n_samples;
    const int i0 = min(lane * Q, S);
    const int64_t base = ray * S;
    const bool want_g = b.d_densities != nullptr || b.d_weights != nullptr;
    const bool use_n = b.up_depth != nullptr && want_g, use_rgb = b.up_rgb != nullptr;
    const RaySums s = ray_sums(p, p.weights, base, i0, min(i0 + Q, S), use_n, false);
    float dc[3] = {0.0f, 0.0f, 0.0f}, bg_term = 0.0f, bg[3] = {0.0f, 0.0f, 0.0f};
    if (use_rgb) {
        dc[0] = b.up_rgb[ray * 3 + 0], dc[1] = b.up_rgb[ray * 3 + 1], dc[2] = b.up_rgb[ray * 3 + 2];
        if (p.background != rr::kBgNone) {
            background_of(p, base, bg);
            bg_term = (dc[0] * bg[0] + dc[1] * bg[1]) + dc[2] * bg[2];
        }
    }
    if (b.d_rgb) {                                                 // d rgb_i = w_i dRGB, + (1 - A) dRGB on the last sample
        const float rest = 1.0f - s.a;
#pragma unroll
        for (int k = 0; k < Q; ++k) {
            const int i = i0 + k;
            if (i >= S) continue;
            const float wi = p.weights[base + i];
            for (int c = 0; c < 3; ++c) {
                float v = wi * dc[c];
                if (p.background == rr::kBgLastSample && i == S - 1) v = v + rest * dc[c];
                b.d_rgb[(base + i) * 3 + c] = v;
            }
        }
    }
    if (!want_g) return;
    const float d_acc = b.up_accumulation ? b.up_accumulation[ray] : 0.0f;
    const float d_dep = use_n ? b.up_depth[ray] : 0.0f;
    const float dn = use_n ? rr::d_depth_d_n(s.a) : 0.0f, da = use_n ? rr::d_depth_d_a(s.n, s.a) : 0.0f;
    // g_i: each consumer's term is one float, formed as that consumer alone forms it, and the terms are added in the order
    // weights, feature, accumulation, expected depth, rgb (a term that is absent is skipped)
    float g[Q];
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        const int i = i0 + k;
        g[k] = 0.0f;
        if (i >= S) continue;
        float v = b.up_weights ? b.up_weights[base + i] : 0.0f;
        if (b.partial) {
            const float* row = b.partial + ray * p.chunks * S + i;
            float f = row[0];
            for (int c = 1; c < p.chunks; ++c) f = f + row[(int64_t)c * S];
            v = v + f;
        }
        if (b.up_accumulation) v = v + d_acc;
        if (use_n) v = v + d_dep * rr::d_depth_d_weight(rr::midpoint(p.starts[base + i], p.ends[base + i]), dn, da);
        if (use_rgb) {
            const float* c = p.rgb + (base + i) * 3;
            float t = (dc[0] * c[0] + dc[1] * c[1]) + dc[2] * c[2];
            if (p.background != rr::kBgNone) t = t - bg_term;
            v = v + t;
        }
        g[k] = v;
    }
    if (!p.densities) {
#pragma unroll
        for (int k = 0; k < Q; ++k)
            if (i0 + k < S) b.d_weights[base + i0 + k] = g[k];
        return;
    }
    float xs[Q];
    float local = 0.0f;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        xs[k] = 0.0f;
        if (i0 + k < S) {
            xs[k] = rr::optical_depth(p.deltas[base + i0 + k], p.densities[base + i0 + k]);
            local = local + xs[k];
        }
    }
    float prefix = wave_exclusive_prefix(local, lane);
    float own[Q], gw[Q];
    float tail = 0.0f;
#pragma unroll
    for (int k = 0; k < Q; ++k) {
        own[k] = 0.0f, gw[k] = 0.0f;
        if (i0 + k < S) {
            const bool masked = rr::replaced(rr::raw_weight(rr::alpha_of(xs[k]), rr::transmittance(prefix)));
            const float gi = masked ? 0.0f : g[k];
            own[k] = rr::d_x_own(gi, xs[k], prefix, masked);
            gw[k] = masked ? 0.0f : gi * p.weights[base + i0 + k];
            prefix = prefix + xs[k];
        }
    }
#pragma unroll
    for (int k = Q - 1; k >= 0; --k) tail = tail + gw[k];
    float after = wave_exclusive_suffix(tail, lane);               // sum of g w over the lanes above
#pragma unroll
    for (int k = Q - 1; k >= 0; --k) {
        if (i0 + k < S) {
            b.d_densities[base + i0 + k] = p.deltas[base + i0 + k] * (own[k] - after);
            after = after + gw[k];
        }
    }
}

// ---- feature forward: out[r, c] = sum_i w[r, i] f[r, i, c] -------------------------------------------------------------------
constexpr int kRows = 4;     // rows of `features` in flight per lane
typedef float v4f __attribute__((ext_vector_type(4)));
__device__ inline v4f zero4() { return v4f{0.0f, 0.0f, 0.0f, 0.0f}; }

__global__ __launch_bounds__(kBlock) void feature_forward_kernel(const float* __restrict__ weights, const float* __restrict__ features,
                                                                 float* __restrict__ out, int64_t n_items, int S, int C, int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t item = __builtin_amdgcn_readfirstlane((int)((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    if (item >= n_items) return;
    const int64_t ray = item / chunks;
    const int ch = (int)(item - ray * chunks) * rr::kChunk + lane * 4;
    if (ch >= C) return;
    const float* w = weights + ray * S;
    const float* f = features + ray * S * C + ch;
    v4f acc = zero4();
    int i = 0;
    for (; i + kRows <= S; i += kRows) {
        v4f row[kRows];
#pragma unroll
        for (int k = 0; k < kRows; ++k) row[k] = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(f + (int64_t)(i + k) * C));
#pragma unroll
        for (int k = 0; k < kRows; ++k) {
            const float wi = w[i + k];
            acc.x = acc.x + wi * row[k].x, acc.y = acc.y + wi * row[k].y, acc.z = acc.z + wi * row[k].z, acc.w = acc.w + wi * row[k].w;
        }
    }
    for (; i < S; ++i) {
        const v4f row = __builtin_nontemporal_load(reinterpret_cast<const v4f*>(f + (int64_t)i * C));
        const float wi = w[i];
        acc.x = acc.x + wi * row.x, acc.y = acc.y + wi * row.y, acc.z = acc.z + wi * row.z, acc.w = acc.w + wi * row.w;
    }
    *reinterpret_cast<v4f*>(out + ray * C + ch) = acc;
}

// ---- feature backward: d_features[r, i, :] = w[r, i] dOut[r, :], partial[r, chunk, i] = sum_{c in chunk} f[r, i, c] dOut[r, c] -----
__device__ inline float dot4(const v4f& a, const v4f& b) { return ((a.x * b.x + a.y * b.y) + a.z * b.z) + a.w * b.w; }

__global__ __launch_bounds__(kBlock) void feature_backward_kernel(const float* __restrict__ weights, const float* __restrict__ features,
                                                                  const float* __restrict__ d_out, float* __restrict__ d_features,
                                                                  float* __restrict__ partial, int64_t n_items, int S, int C, int chunks) {
    const int lane = threadIdx.x & 63;
    const int64_t item = __builtin_amdgcn_readfirstlane((int)((int64_t)blockIdx.x * kWavesPerBlock + (threadIdx.x >> 6)));
    if (item >= n_items) return;
    const int64_t ray = item / chunks;
    const int ch = (int)(item - ray * chunks) * rr::kChunk + lane * 4;
    const bool live = ch < C;                                      // lanes past C stay for the wave sums and add zeros
    const int64_t at = ray * S * C + (live ? ch : 0);
    const float* w = weights + ray * S;
    const v4f d = live ? *reinterpret_cast<const v4f*>(d_out + ray * C + ch) : zero4();
    float* part = partial ? partial + item * S : nullptr;
    int i = 0;
    for (; i + kRows <= S; i += kRows) {
        float dots[kRows];
        if (partial) {
            v4f row[kRows];
#pragma unroll
            for (int k = 0; k < kRows; ++k)
                row[k] = live ? __builtin_nontemporal_load(reinterpret_cast<const v4f*>(features + at + (int64_t)(i + k) * C))
                              : zero4();
#pragma unroll
            for (int k = 0; k < kRows; ++k) dots[k] = dot4(row[k], d);
        }
        if (d_features && live) {
#pragma unroll
            for (int k = 0; k < kRows; ++k) {
                const float wi = w[i + k];
                __builtin_nontemporal_store(v4f{wi * d.x, wi * d.y, wi * d.z, wi * d.w},
                                            reinterpret_cast<v4f*>(d_features + at + (int64_t)(i + k) * C));
            }
        }
        if (partial) {
#pragma unroll
            for (int m = 32; m >= 1; m >>= 1) {
#pragma unroll
                for (int k = 0; k < kRows; ++k) dots[k] = dots[k] + __shfl_xor(dots[k], m, 64);
            }
            if (lane < kRows) part[i + lane] = lane == 0 ? dots[0] : lane == 1 ? dots[1] : lane == 2 ? dots[2] : dots[3];
        }
    }
    for (; i < S; ++i) {
        if (d_features && live) {
            const float wi = w[i];
            __builtin_nontemporal_store(v4f{wi * d.x, wi * d.y, wi * d.z, wi * d.w},
                                        reinterpret_cast<v4f*>(d_features + at + (int64_t)i * C));
        }
        if (partial) {
            const v4f row = live ? __builtin_nontemporal_load(reinterpret_cast<const v4f*>(features + at + (int64_t)i * C))
                                    : zero4();
            const float dot = wave_sum(dot4(row, d));
            if (lane == 0) part[i] = dot;
        }
    }
}

// ---- host side --------------------------------------------------------------------------------------------------------------
int check_desc(const pixie_ray_desc* desc, const char* who) {
    PX_REQUIRE(desc != nullptr, "%s: desc is NULL", who);
    PX_REQUIRE(desc->n_rays >= 1 && desc->n_rays <= rr::kMaxRays, "%s: n_rays %lld outside [1, 2^24]", who, (long long)desc->n_rays);
    PX_REQUIRE(desc->n_samples >= 1 && desc->n_samples <= rr::kMaxSamples, "%s: n_samples %d outside [1, %d]", who, desc->n_samples,
               rr::kMaxSamples);
    PX_REQUIRE(desc->n_channels >= 0 && desc->n_channels <= rr::kMaxChannels && desc->n_channels % 4 == 0,
               "%s: n_channels %d must be a multiple of 4 in [0, %d]", who, desc->n_channels, rr::kMaxChannels);
    PX_REQUIRE(desc->n_channels == 0 || desc->n_samples <= rr::kMaxFeatureSamples, "%s: n_samples %d above %d with features", who,
               desc->n_samples, rr::kMaxFeatureSamples);
    PX_REQUIRE(desc->background >= rr::kBgNone && desc->background <= rr::kBgLastSample, "%s: background mode %d", who, desc->background);
    return 0;
}

RayParams params_of(const pixie_ray_desc* desc, const pixie_ray_inputs* in) {
    RayParams p;
    p.densities = in->d_densities, p.deltas = in->d_deltas, p.weights = in->d_weights, p.starts = in->d_starts, p.ends = in->d_ends;
    p.rgb = in->d_rgb;
    p.n_rays = desc->n_rays, p.n_samples = desc->n_samples, p.per_lane = rr::samples_per_lane(desc->n_samples);
    p.chunks = rr::chunks_of(desc->n_channels), p.background = desc->background;
    p.bg[0] = desc->bg[0], p.bg[1] = desc->bg[1], p.bg[2] = desc->bg[2];
    return p;
}

bool aligned16(const void* ptr) { return (reinterpret_cast<uintptr_t>(ptr) & 15) == 0; }

int64_t scratch_bytes_of(const pixie_ray_desc* desc) {
    return 4 * desc->n_rays * (int64_t)rr::chunks_of(desc->n_channels) * desc->n_samples;
}

template <int Q>
void launch_ray_backward(const RayParams& p, const RayBackwardArgs& b, hipStream_t st) {
    hipLaunchKernelGGL(ray_backward_kernel<Q>, dim3(cdiv(p.n_rays, kWavesPerBlock)), dim3(kBlock), 0, st, p, b);
}

}  // namespace
}  // namespace pixie

using namespace pixie;

extern "C" int pixie_ray_composite_bytes(const pixie_ray_desc* desc, int64_t* scratch_bytes) {
    if (int rc = check_desc(desc, "pixie_ray_composite_bytes")) return rc;
    PX_REQUIRE(scratch_bytes != nullptr, "pixie_ray_composite_bytes: scratch_bytes is NULL");
    *scratch_bytes = scratch_bytes_of(desc);
    return 0;
}

extern "C" int pixie_ray_composite_forward(const pixie_ray_desc* desc, const pixie_ray_inputs* in, const pixie_ray_outputs* out, void* stream) {
    const char* who = "pixie_ray_composite_forward";
    if (int rc = check_desc(desc, who)) return rc;
    PX_REQUIRE(in != nullptr && out != nullptr, "%s: NULL argument", who);
    const bool density_mode = in->d_densities != nullptr;
    if (density_mode) {
        PX_REQUIRE(in->d_deltas != nullptr && in->d_weights == nullptr && out->d_weights != nullptr,
                   "%s: densities need deltas and a weights output, and exclude given weights", who);
    } else {
        PX_REQUIRE(in->d_weights != nullptr && out->d_weights == nullptr, "%s: without densities the weights are an input, not an output", who);
    }
    PX_REQUIRE((in->d_starts == nullptr) == (in->d_ends == nullptr), "%s: starts and ends go together", who);
    PX_REQUIRE(!(out->d_expected_depth || out->d_median_depth) || in->d_starts, "%s: a depth output needs starts and ends", who);
    PX_REQUIRE(!out->d_rgb || in->d_rgb, "%s: the rgb output needs the samples' rgb", who);
    PX_REQUIRE(!out->d_feature || (in->d_features && desc->n_channels > 0), "%s: the feature output needs features and n_channels > 0", who);
    PX_REQUIRE(aligned16(in->d_features) && aligned16(out->d_feature), "%s: feature arrays must be 16-byte aligned", who);
    hipStream_t st = as_stream(stream);
    RayParams p = params_of(desc, in);
    RayForwardOut o = {out->d_weights, out->d_accumulation, out->d_expected_depth, out->d_median_depth, out->d_rgb};
    if (density_mode || o.accumulation || o.expected_depth || o.median_depth || o.rgb) {
        hipLaunchKernelGGL(ray_forward_kernel, dim3(cdiv(p.n_rays, kWavesPerBlock)), dim3(kBlock), 0, st, p, o);
        PX_CHECK_HIP(hipGetLastError());
    }
    if (out->d_feature) {
        const int64_t items = desc->n_rays * p.chunks;
        hipLaunchKernelGGL(feature_forward_kernel, dim3(cdiv(items, kWavesPerBlock)), dim3(kBlock), 0, st,
                           density_mode ? out->d_weights : in->d_weights, in->d_features, out->d_feature, items, desc->n_samples,
                           desc->n_channels, p.chunks);
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int pixie_ray_composite_backward(const pixie_ray_desc* desc, const pixie_ray_inputs* in, const pixie_ray_upstream* up,
                                            const pixie_ray_grads* grads, void* d_scratch, void* stream) {
    const char* who = "pixie_ray_composite_backward";
    if (int rc = check_desc(desc, who)) return rc;
    PX_REQUIRE(in != nullptr && up != nullptr && grads != nullptr, "%s: NULL argument", who);
    PX_REQUIRE(in->d_weights != nullptr, "%s: the weights (given, or the forward's output) are required", who);
    const bool density_mode = in->d_densities != nullptr;
    if (density_mode) {
        PX_REQUIRE(in->d_deltas != nullptr && grads->d_weights == nullptr, "%s: densities need deltas; their gradient is d_densities", who);
    } else {
        PX_REQUIRE(grads->d_densities == nullptr && up->d_weights == nullptr, "%s: without densities there is no weights output", who);
    }
    PX_REQUIRE((in->d_starts == nullptr) == (in->d_ends == nullptr), "%s: starts and ends go together", who);
    PX_REQUIRE(!up->d_expected_depth || in->d_starts, "%s: the expected depth's gradient needs starts and ends", who);
    PX_REQUIRE(!up->d_rgb || in->d_rgb, "%s: the rgb gradient needs the samples' rgb", who);
    PX_REQUIRE(!grads->d_rgb || up->d_rgb, "%s: d_rgb needs the rgb output's gradient", who);
    PX_REQUIRE(!up->d_feature || (in->d_features && desc->n_channels > 0), "%s: the feature gradient needs features and n_channels > 0", who);
    PX_REQUIRE(!grads->d_features || up->d_feature, "%s: d_features needs the feature output's gradient", who);
    PX_REQUIRE(aligned16(in->d_features) && aligned16(up->d_feature) && aligned16(grads->d_features), "%s: feature arrays must be 16-byte aligned", who);
    const bool want_g = grads->d_densities || grads->d_weights;
    const bool want_partial = want_g && up->d_feature;
    PX_REQUIRE(!want_partial || d_scratch, "%s: d_scratch is NULL", who);
    hipStream_t st = as_stream(stream);
    RayParams p = params_of(desc, in);
    if (up->d_feature && (grads->d_features || want_partial)) {
        const int64_t items = desc->n_rays * p.chunks;
        hipLaunchKernelGGL(feature_backward_kernel, dim3(cdiv(items, kWavesPerBlock)), dim3(kBlock), 0, st, in->d_weights, in->d_features,
                           up->d_feature, grads->d_features, want_partial ? (float*)d_scratch : nullptr, items, desc->n_samples,
                           desc->n_channels, p.chunks);
        PX_CHECK_HIP(hipGetLastError());
    }
    if (want_g || grads->d_rgb) {
        RayBackwardArgs b = {up->d_weights, up->d_accumulation, up->d_expected_depth, up->d_rgb, want_partial ? (const float*)d_scratch : nullptr,
                             grads->d_densities, grads->d_weights, grads->d_rgb};
        switch (p.per_lane) {
#define PIXIE_RAY_Q(Q) case Q: launch_ray_backward<Q>(p, b, st); break;
            PIXIE_RAY_Q(1) PIXIE_RAY_Q(2) PIXIE_RAY_Q(3) PIXIE_RAY_Q(4) PIXIE_RAY_Q(5) PIXIE_RAY_Q(6) PIXIE_RAY_Q(7) PIXIE_RAY_Q(8)
            PIXIE_RAY_Q(9) PIXIE_RAY_Q(10) PIXIE_RAY_Q(11) PIXIE_RAY_Q(12) PIXIE_RAY_Q(13) PIXIE_RAY_Q(14) PIXIE_RAY_Q(15) PIXIE_RAY_Q(16)
#undef PIXIE_RAY_Q
            default: return set_error("%s: %d samples per lane", who, p.per_lane);
        }
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}
