// pixie_amd/csrc/ray_sample.hip -- proposal sampling and its two losses: the SpacedSampler family, PDFSampler.generate_ray_samples,
// Frustums.get_positions, interlevel_loss and distortion_loss with their backward passes (include/pixie_hip.h).
//
// One wave per ray, one ray per 64-thread workgroup.  A ray's edges, cdf and weights are staged in LDS (at most 1025 floats
// each), where the binary searches of searchsorted read them; a lane sums q = ceil(S / 64) consecutive samples sequentially and the
// lanes' sums are scanned or reduced over the wave in a fixed order (wave_order.h), so no result depends on the launch geometry or on
// the other rays.  The two losses write one float per ray (and level) and a one-workgroup finalise adds those in double, in a fixed
// order.  The interlevel backward gathers: the fine intervals whose [lo, hi] covers proposal interval j are contiguous because lo and
// hi are monotone, and are summed in index order.  No floating-point atomics, no synchronise, no host read-back.
// Built with -ffp-contract=off: the per-sample arithmetic is ray_sample_math.h as g++ rounds it.
#include "../../include/pixie_hip.h"
#include "common.h"
#include "ray_sample_math.h"
#include "wave_order.h"

namespace pixie {
namespace {

constexpr int kWave = 64;                  // threads per workgroup: one wave, so __syncthreads orders the wave's own LDS traffic
constexpr int kEdges = rs::kMaxSamples + 1;
constexpr int kFinaliseBlock = 256;

__device__ inline float wave_exclusive_max(float v, int lane) {     // the largest value of the lanes below, 0 for lane 0
    float inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = rs::running_max(o, inc);
    }
    const float below = __shfl_up(inc, 1, 64);
    return lane == 0 ? 0.0f : below;
}

// ---- what both samplers write from a ray's spacing bins --------------------------------------------------------------------------
struct EmitArgs {
    const float* origins;       // (R, 3) or nullptr
    const float* directions;    // (R, 3)
    float* bins;                // (R, M + 1) spacing bins
    float* starts;              // (R, M) euclidean
    float* ends;
    float* deltas;
    float* positions;           // (R, M, 3)
    int spacing;
};

__device__ inline void emit(const EmitArgs& a, const float* s_bins, int n_out, float s_near, float s_far, int64_t ray, int lane) {
    if (a.bins)
        for (int k = lane; k <= n_out; k += kWave) a.bins[ray * (n_out + 1) + k] = s_bins[k];
    if (a.spacing == rs::kForeign) return;
    float o[3] = {0.0f, 0.0f, 0.0f}, d[3] = {0.0f, 0.0f, 0.0f};
    if (a.positions)
        for (int c = 0; c < 3; ++c) o[c] = a.origins[ray * 3 + c], d[c] = a.directions[ray * 3 + c];
    const int64_t base = ray * n_out;
    for (int k = lane; k < n_out; k += kWave) {
        const float start = rs::to_euclidean(a.spacing, s_bins[k], s_near, s_far);
        const float end = rs::to_euclidean(a.spacing, s_bins[k + 1], s_near, s_far);
        if (a.starts) a.starts[base + k] = start;
        if (a.ends) a.ends[base + k] = end;
        if (a.deltas) a.deltas[base + k] = rs::delta_of(start, end);
        if (a.positions)
            for (int c = 0; c < 3; ++c) a.positions[(base + k) * 3 + c] = rs::position(o[c], d[c], start, end);
    }
}

// ---- SpacedSampler ------------------------------------------------------------------------------------------------------------------
struct SpacedArgs {
    const float* nears;         // (R)
    const float* fars;
    const float* table;         // (S + 1) linspace(0, 1, S + 1)
    const float* jitter;        // (R, jitter_stride) or nullptr
    float* s_near;              // (R) or nullptr
    float* s_far;
    int n_samples, jitter_stride;
};

__global__ __launch_bounds__(kWave) void spaced_kernel(SpacedArgs p, EmitArgs e) {
    __shared__ float s_bins[kEdges];
    const int lane = threadIdx.x;
    const int64_t ray = blockIdx.x;
    const int S = p.n_samples;
    for (int k = lane; k <= S; k += kWave) {
        float b = p.table[k];
        if (p.jitter) b = rs::stratified_bin(p.table, k, S, p.jitter[ray * p.jitter_stride + (p.jitter_stride == 1 ? 0 : k)]);
        s_bins[k] = b;
    }
    __syncthreads();
    const float s_near = rs::spacing_fn(e.spacing, p.nears[ray]), s_far = rs::spacing_fn(e.spacing, p.fars[ray]);
    if (lane == 0) {
        if (p.s_near) p.s_near[ray] = s_near;
        if (p.s_far) p.s_far[ray] = s_far;
    }
    emit(e, s_bins, S, s_near, s_far, ray, lane);
}

// ---- PDFSampler ---------------------------------------------------------------------------------------------------------------------
struct PdfArgs {
    const float* existing;      // (R, S + 1) spacing bins of the existing samples
    const float* weights;       // (R, S)
    const float* table;         // (N + 1) linspace(0, 1 - 1 / (N + 1), N + 1)
    const float* jitter;        // (R, jitter_stride) or nullptr
    const float* s_near;        // (R), unless the spacing is foreign
    const float* s_far;
    int n_existing, n_new, jitter_stride, include_original;
    float padding, eps, anneal, u_scale, u_offset;
};

__global__ __launch_bounds__(kWave) void pdf_kernel(PdfArgs p, EmitArgs e) {
    __shared__ float s_cdf[kEdges], s_old[kEdges], s_new[kEdges];
    const int lane = threadIdx.x;
    const int64_t ray = blockIdx.x;
    const int S = p.n_existing, n_u = p.n_new + 1;
    const int q = rs::samples_per_lane(S);
    const int i0 = min(lane * q, S), i1 = min(i0 + q, S);
    const float* w = p.weights + ray * S;
    for (int k = lane; k <= S; k += kWave) s_old[k] = p.existing[ray * (S + 1) + k];
    // the padded histogram: a lane keeps its own entries in s_cdf[i + 1] until it overwrites them with the cdf
    float local = 0.0f;
    for (int i = i0; i < i1; ++i) {
        const float h = rs::histogram_weight(w[i], p.anneal, p.padding);
        s_cdf[i + 1] = h;
        local = local + h;
    }
    const float sum = wave_sum(local);
    const float pad = rs::empty_padding(sum, p.eps);
    const float share = pad / (float)S, total = sum + pad;
    local = 0.0f;
    for (int i = i0; i < i1; ++i) local = local + rs::pdf_of(s_cdf[i + 1], share, total);
    float running = wave_exclusive_prefix(local, lane);
    float top = 0.0f;
    for (int i = i0; i < i1; ++i) {
        running = running + rs::pdf_of(s_cdf[i + 1], share, total);
        top = rs::running_max(top, rs::cdf_clamp(running));
        s_cdf[i + 1] = top;
    }
    // a lane's chain and the scan round differently, so a lane may start an ulp below the lane before it: the running maximum over
    // the lanes makes the cdf non-decreasing, which the binary search and the order of the new bins rely on
    const float floor_ = wave_exclusive_max(top, lane);
    for (int i = i0; i < i1; ++i) s_cdf[i + 1] = rs::running_max(floor_, s_cdf[i + 1]);
    if (lane == 0) s_cdf[0] = 0.0f;
    __syncthreads();
    for (int k = lane; k < n_u; k += kWave) {
        const float u = p.table[k] + (p.jitter ? p.jitter[ray * p.jitter_stride + (p.jitter_stride == 1 ? 0 : k)] * p.u_scale : p.u_offset);
        const int inds = rs::count_le(s_cdf, S + 1, u);
        const int below = rs::clamp_index(inds - 1, 0, S), above = rs::clamp_index(inds, 0, S);
        s_new[k] = rs::cdf_interp(u, s_cdf[below], s_cdf[above], s_old[below], s_old[above]);
    }
    __syncthreads();
    const float s_near = e.spacing == rs::kForeign ? 0.0f : p.s_near[ray], s_far = e.spacing == rs::kForeign ? 0.0f : p.s_far[ray];
    if (!p.include_original) {
        emit(e, s_new, p.n_new, s_near, s_far, ray, lane);
        return;
    }
    // both lists are sorted: an element's place in the merge is its own index plus the number of the other list's elements before
    // it (an existing edge goes before a new bin of the same value).  The cdf is no longer needed: the merge takes its place.
    for (int k = lane; k < n_u; k += kWave) s_cdf[k + rs::count_le(s_old, S + 1, s_new[k])] = s_new[k];
    for (int i = lane; i <= S; i += kWave) s_cdf[i + rs::count_lt(s_new, n_u, s_old[i])] = s_old[i];
    __syncthreads();
    emit(e, s_cdf, p.n_new + S + 1, s_near, s_far, ray, lane);
}

// ---- interlevel loss ----------------------------------------------------------------------------------------------------------------
struct InterArgs {
    const float* fine_edges;    // (R, S + 1)
    const float* fine_weights;  // (R, S)
    const float* edges[rs::kMaxLevels];       // (R, S_l + 1)
    const float* weights[rs::kMaxLevels];     // (R, S_l)
    float* grads[rs::kMaxLevels];             // (R, S_l) or nullptr (backward)
    int n_env[rs::kMaxLevels];
    int64_t n_rays;
    int n_fine;
    float* per_sample;          // (R, S) or nullptr: lossfun_outer's own output, one level (forward)
    int up_per_sample;          // backward: the upstream gradient is (R, S), not one float
};

// the level's edges and weights and the fine edges, into LDS
__device__ inline void stage_level(const InterArgs& p, int level, int64_t ray, int lane, float* s_env, float* s_w, float* s_fine) {
    const int n = p.n_env[level], S = p.n_fine;
    const float* edges = p.edges[level] + ray * (n + 1);
    const float* w = p.weights[level] + ray * n;
    for (int k = lane; k <= n; k += kWave) s_env[k] = edges[k];
    for (int k = lane; k <= S; k += kWave) s_fine[k] = p.fine_edges[ray * (S + 1) + k];
    for (int k = lane; k < n; k += kWave) s_w[k] = w[k];
    __syncthreads();
}

__global__ __launch_bounds__(kWave) void interlevel_forward_kernel(InterArgs p, float* partial) {
    __shared__ float s_env[kEdges], s_w[kEdges], s_fine[kEdges];
    const int lane = threadIdx.x, level = blockIdx.y;
    const int64_t ray = blockIdx.x;
    stage_level(p, level, ray, lane, s_env, s_w, s_fine);
    const int S = p.n_fine, n = p.n_env[level];
    const int q = rs::samples_per_lane(S);
    const int i0 = min(lane * q, S), i1 = min(i0 + q, S);
    float local = 0.0f;
    for (int i = i0; i < i1; ++i) {
        const int lo = rs::outer_lo(s_env, n, s_fine[i]), hi = rs::outer_hi(s_env, n, s_fine[i + 1]);
        const float term = rs::outer_term(p.fine_weights[ray * S + i], rs::outer_sum(s_w, lo, hi));
        if (p.per_sample) p.per_sample[ray * S + i] = term;
        local = local + term;
    }
    const float total = wave_sum(local);
    if (partial && lane == 0) partial[(int64_t)level * p.n_rays + ray] = total;
}

__global__ __launch_bounds__(kWave) void interlevel_backward_kernel(InterArgs p, const float* upstream, float count) {
    __shared__ float s_env[kEdges], s_w[kEdges], s_fine[kEdges], s_g[rs::kMaxSamples];
    __shared__ int s_lo[rs::kMaxSamples], s_hi[rs::kMaxSamples];
    const int lane = threadIdx.x, level = blockIdx.y;
    if (p.grads[level] == nullptr) return;                         // the whole workgroup leaves before any barrier
    const int64_t ray = blockIdx.x;
    stage_level(p, level, ray, lane, s_env, s_w, s_fine);
    const int S = p.n_fine, n = p.n_env[level];
    const float mean_scale = p.up_per_sample ? 0.0f : upstream[0] / count;
    for (int i = lane; i < S; i += kWave) {
        const float scale = p.up_per_sample ? upstream[ray * S + i] : mean_scale;
        const int lo = rs::outer_lo(s_env, n, s_fine[i]), hi = rs::outer_hi(s_env, n, s_fine[i + 1]);
        s_lo[i] = lo, s_hi[i] = hi;
        s_g[i] = rs::outer_term_grad(p.fine_weights[ray * S + i], rs::outer_sum(s_w, lo, hi), scale);
    }
    __syncthreads();
    float* grad = p.grads[level] + ray * n;
    for (int j = lane; j < n; j += kWave) {
        int a = 0, b = S;                                          // first i with hi_i >= j
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (s_hi[mid] < j) a = mid + 1; else b = mid;
        }
        const int first = a;
        a = 0, b = S;                                              // first i with lo_i > j
        while (a < b) {
            const int mid = (a + b) >> 1;
            if (s_lo[mid] <= j) a = mid + 1; else b = mid;
        }
        float g = 0.0f;
        for (int i = first; i < a; ++i)
            if (s_lo[i] <= j && j <= s_hi[i]) g = g + s_g[i];      // always true for sorted edges
        grad[j] = g;
    }
}

// ---- distortion loss ----------------------------------------------------------------------------------------------------------------
__device__ inline void stage_distortion(const float* t, const float* w, int S, int lane, float* s_u, float* s_w) {
    for (int k = lane; k < S; k += kWave) s_u[k] = rs::interval_mid(t[k], t[k + 1]), s_w[k] = w[k];
    __syncthreads();
}
__device__ inline float distortion_inner(const float* s_u, const float* s_w, int S, int i) {
    const float u = s_u[i];
    float inner = 0.0f;
    for (int j = 0; j < S; ++j) inner = inner + rs::distortion_pair(s_w[j], u, s_u[j]);
    return inner;
}

__global__ __launch_bounds__(kWave) void distortion_forward_kernel(const float* edges, const float* weights, int S, float* partial) {
    __shared__ float s_u[rs::kMaxSamples], s_w[rs::kMaxSamples];
    const int lane = threadIdx.x;
    const int64_t ray = blockIdx.x;
    const float* t = edges + ray * (S + 1);
    stage_distortion(t, weights + ray * S, S, lane, s_u, s_w);
    const int q = rs::samples_per_lane(S);
    const int i0 = min(lane * q, S), i1 = min(i0 + q, S);
    float inter = 0.0f, intra = 0.0f;
    for (int i = i0; i < i1; ++i) {
        inter = inter + s_w[i] * distortion_inner(s_u, s_w, S, i);
        intra = intra + rs::distortion_intra(s_w[i], t[i], t[i + 1]);
    }
    inter = wave_sum(inter), intra = wave_sum(intra);
    if (lane == 0) partial[ray] = rs::distortion_ray(inter, intra);
}

__global__ __launch_bounds__(kWave) void distortion_backward_kernel(const float* edges, const float* weights, int S, const float* upstream,
                                                                    int up_per_ray, float count, float* grad) {
    __shared__ float s_u[rs::kMaxSamples], s_w[rs::kMaxSamples];
    const int lane = threadIdx.x;
    const int64_t ray = blockIdx.x;
    const float* t = edges + ray * (S + 1);
    stage_distortion(t, weights + ray * S, S, lane, s_u, s_w);
    const float scale = up_per_ray ? upstream[ray] : upstream[0] / count;
    for (int k = lane; k < S; k += kWave)
        grad[ray * S + k] = rs::distortion_grad(distortion_inner(s_u, s_w, S, k), s_w[k], t[k], t[k + 1], scale);
}

// out[0] = (sum of `count` floats, in double: a fixed stride per thread, then a fixed tree) * inv_count
__global__ __launch_bounds__(kFinaliseBlock) void loss_finalise_kernel(const float* partial, int64_t count, double inv_count, float* out) {
    __shared__ double s_sum[kFinaliseBlock];
    double acc = 0.0;
    for (int64_t k = threadIdx.x; k < count; k += kFinaliseBlock) acc += (double)partial[k];
    s_sum[threadIdx.x] = acc;
    __syncthreads();
    for (int s = kFinaliseBlock / 2; s > 0; s >>= 1) {
        if ((int)threadIdx.x < s) s_sum[threadIdx.x] += s_sum[threadIdx.x + s];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = (float)(s_sum[0] * inv_count);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
int check_rays(int64_t n_rays, const char* who) {
    PX_REQUIRE(n_rays >= 1 && n_rays <= rs::kMaxRays, "%s: n_rays %lld outside [1, 2^24]", who, (long long)n_rays);
    return 0;
}

int check_sample_desc(const pixie_ray_sample_desc* desc, bool pdf, const char* who) {
    PX_REQUIRE(desc != nullptr, "%s: desc is NULL", who);
    if (int rc = check_rays(desc->n_rays, who)) return rc;
    PX_REQUIRE(desc->n_samples >= 1 && desc->n_samples <= rs::kMaxSamples, "%s: n_samples %d outside [1, %d]", who, desc->n_samples,
               rs::kMaxSamples);
    PX_REQUIRE(desc->spacing >= rs::kForeign && desc->spacing <= rs::kPiecewise, "%s: spacing kind %d", who, desc->spacing);
    PX_REQUIRE(desc->jitter_stride == 0 || desc->jitter_stride == 1 || desc->jitter_stride == desc->n_samples + 1,
               "%s: jitter_stride %d must be 0 (no jitter), 1 or n_samples + 1", who, desc->jitter_stride);
    if (pdf) {
        PX_REQUIRE(desc->n_existing >= 1 && desc->n_existing <= rs::kMaxSamples, "%s: n_existing %d outside [1, %d]", who, desc->n_existing,
                   rs::kMaxSamples);
        PX_REQUIRE(!desc->include_original || desc->n_samples + desc->n_existing + 1 <= rs::kMaxSamples,
                   "%s: %d new + %d existing + 1 samples with include_original, above %d", who, desc->n_samples, desc->n_existing,
                   rs::kMaxSamples);
    } else {
        PX_REQUIRE(desc->spacing != rs::kForeign, "%s: the spaced sampler needs a spacing kind", who);
    }
    return 0;
}

int check_emit(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* in, const pixie_ray_sample_outputs* out, const char* who) {
    PX_REQUIRE(out->d_bins || out->d_starts || out->d_ends || out->d_deltas || out->d_positions, "%s: no output is wanted", who);
    PX_REQUIRE(desc->spacing != rs::kForeign || !(out->d_starts || out->d_ends || out->d_deltas || out->d_positions),
               "%s: a foreign spacing function yields the spacing bins alone", who);
    PX_REQUIRE(!out->d_positions || (in->d_origins && in->d_directions), "%s: positions need origins and directions", who);
    PX_REQUIRE(desc->jitter_stride == 0 ? in->d_jitter == nullptr : in->d_jitter != nullptr, "%s: jitter and jitter_stride go together", who);
    PX_REQUIRE(in->d_table != nullptr, "%s: the linspace table is required", who);
    return 0;
}

EmitArgs emit_of(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* in, const pixie_ray_sample_outputs* out) {
    return EmitArgs{in->d_origins, in->d_directions, out->d_bins, out->d_starts, out->d_ends, out->d_deltas, out->d_positions, desc->spacing};
}

int check_interlevel(const pixie_ray_interlevel_desc* desc, const char* who) {
    PX_REQUIRE(desc != nullptr, "%s: desc is NULL", who);
    if (int rc = check_rays(desc->n_rays, who)) return rc;
    PX_REQUIRE(desc->n_fine >= 1 && desc->n_fine <= rs::kMaxSamples, "%s: n_fine %d outside [1, %d]", who, desc->n_fine, rs::kMaxSamples);
    PX_REQUIRE(desc->n_levels >= 1 && desc->n_levels <= rs::kMaxLevels, "%s: n_levels %d outside [1, %d]", who, desc->n_levels, rs::kMaxLevels);
    for (int l = 0; l < desc->n_levels; ++l)
        PX_REQUIRE(desc->n_proposal[l] >= 1 && desc->n_proposal[l] <= rs::kMaxSamples, "%s: level %d has %d samples, outside [1, %d]", who, l,
                   desc->n_proposal[l], rs::kMaxSamples);
    PX_REQUIRE(!desc->per_sample || desc->n_levels == 1, "%s: per_sample is for one level", who);
    return 0;
}

int inter_args(const pixie_ray_interlevel_desc* desc, const pixie_ray_interlevel_inputs* in, const char* who, InterArgs* p) {
    PX_REQUIRE(in != nullptr && in->d_fine_edges && in->d_fine_weights, "%s: the fine level's edges and weights are required", who);
    p->fine_edges = in->d_fine_edges, p->fine_weights = in->d_fine_weights, p->n_rays = desc->n_rays, p->n_fine = desc->n_fine;
    for (int l = 0; l < rs::kMaxLevels; ++l) {
        const bool live = l < desc->n_levels;
        PX_REQUIRE(!live || (in->d_edges[l] && in->d_weights[l]), "%s: level %d needs edges and weights", who, l);
        p->edges[l] = live ? in->d_edges[l] : nullptr, p->weights[l] = live ? in->d_weights[l] : nullptr;
        p->grads[l] = nullptr, p->n_env[l] = live ? desc->n_proposal[l] : 0;
    }
    p->per_sample = nullptr, p->up_per_sample = desc->per_sample;
    return 0;
}

int check_distortion(const pixie_ray_distortion_desc* desc, const char* who) {
    PX_REQUIRE(desc != nullptr, "%s: desc is NULL", who);
    if (int rc = check_rays(desc->n_rays, who)) return rc;
    PX_REQUIRE(desc->n_samples >= 1 && desc->n_samples <= rs::kMaxSamples, "%s: n_samples %d outside [1, %d]", who, desc->n_samples,
               rs::kMaxSamples);
    return 0;
}

}  // namespace
}  // namespace pixie

using namespace pixie;

extern "C" int pixie_ray_sample_spaced(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* in, const pixie_ray_sample_outputs* out,
                                       void* stream) {
    const char* who = "pixie_ray_sample_spaced";
    if (int rc = check_sample_desc(desc, false, who)) return rc;
    PX_REQUIRE(in != nullptr && out != nullptr, "%s: NULL argument", who);
    if (int rc = check_emit(desc, in, out, who)) return rc;
    PX_REQUIRE(in->d_nears && in->d_fars, "%s: nears and fars are required", who);
    SpacedArgs p = {in->d_nears, in->d_fars, in->d_table, in->d_jitter, out->d_s_near, out->d_s_far, desc->n_samples, desc->jitter_stride};
    hipLaunchKernelGGL(spaced_kernel, dim3((unsigned)desc->n_rays), dim3(kWave), 0, as_stream(stream), p, emit_of(desc, in, out));
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_ray_sample_pdf(const pixie_ray_sample_desc* desc, const pixie_ray_sample_inputs* in, const pixie_ray_sample_outputs* out,
                                    void* stream) {
    const char* who = "pixie_ray_sample_pdf";
    if (int rc = check_sample_desc(desc, true, who)) return rc;
    PX_REQUIRE(in != nullptr && out != nullptr, "%s: NULL argument", who);
    if (int rc = check_emit(desc, in, out, who)) return rc;
    PX_REQUIRE(in->d_existing_bins && in->d_weights, "%s: the existing bins and their weights are required", who);
    PX_REQUIRE(desc->spacing == rs::kForeign || (in->d_s_near && in->d_s_far), "%s: a spacing kind needs s_near and s_far", who);
    PX_REQUIRE(out->d_s_near == nullptr && out->d_s_far == nullptr, "%s: s_near and s_far are inputs here", who);
    PdfArgs p = {in->d_existing_bins, in->d_weights, in->d_table, in->d_jitter, in->d_s_near, in->d_s_far, desc->n_existing, desc->n_samples,
                 desc->jitter_stride, desc->include_original, desc->histogram_padding, desc->eps, desc->anneal, desc->u_scale, desc->u_offset};
    hipLaunchKernelGGL(pdf_kernel, dim3((unsigned)desc->n_rays), dim3(kWave), 0, as_stream(stream), p, emit_of(desc, in, out));
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_ray_interlevel_bytes(const pixie_ray_interlevel_desc* desc, int64_t* scratch_bytes) {
    if (int rc = check_interlevel(desc, "pixie_ray_interlevel_bytes")) return rc;
    PX_REQUIRE(scratch_bytes != nullptr, "pixie_ray_interlevel_bytes: scratch_bytes is NULL");
    *scratch_bytes = 4 * desc->n_rays * desc->n_levels;
    return 0;
}

extern "C" int pixie_ray_interlevel_forward(const pixie_ray_interlevel_desc* desc, const pixie_ray_interlevel_inputs* in, float* d_loss,
                                            float* d_per_sample, void* d_scratch, void* stream) {
    const char* who = "pixie_ray_interlevel_forward";
    if (int rc = check_interlevel(desc, who)) return rc;
    InterArgs p;
    if (int rc = inter_args(desc, in, who, &p)) return rc;
    hipStream_t st = as_stream(stream);
    if (desc->per_sample) {
        PX_REQUIRE(d_per_sample != nullptr && d_loss == nullptr, "%s: per_sample writes d_per_sample and no d_loss", who);
        p.per_sample = d_per_sample;
        hipLaunchKernelGGL(interlevel_forward_kernel, dim3((unsigned)desc->n_rays, 1), dim3(kWave), 0, st, p, (float*)nullptr);
        PX_CHECK_HIP(hipGetLastError());
        return 0;
    }
    PX_REQUIRE(d_loss != nullptr && d_scratch != nullptr && d_per_sample == nullptr, "%s: the mean needs d_loss and d_scratch, and no d_per_sample", who);
    hipLaunchKernelGGL(interlevel_forward_kernel, dim3((unsigned)desc->n_rays, (unsigned)desc->n_levels), dim3(kWave), 0, st, p, (float*)d_scratch);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(loss_finalise_kernel, dim3(1), dim3(kFinaliseBlock), 0, st, (const float*)d_scratch, desc->n_rays * desc->n_levels,
                       1.0 / ((double)desc->n_rays * desc->n_fine), d_loss);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_ray_interlevel_backward(const pixie_ray_interlevel_desc* desc, const pixie_ray_interlevel_inputs* in, const float* d_upstream,
                                             const pixie_ray_interlevel_grads* grads, void* stream) {
    const char* who = "pixie_ray_interlevel_backward";
    if (int rc = check_interlevel(desc, who)) return rc;
    InterArgs p;
    if (int rc = inter_args(desc, in, who, &p)) return rc;
    PX_REQUIRE(d_upstream != nullptr && grads != nullptr, "%s: d_upstream or grads is NULL", who);
    bool any = false;
    for (int l = 0; l < desc->n_levels; ++l) p.grads[l] = grads->d_weights[l], any = any || grads->d_weights[l];
    if (!any) return 0;
    hipLaunchKernelGGL(interlevel_backward_kernel, dim3((unsigned)desc->n_rays, (unsigned)desc->n_levels), dim3(kWave), 0, as_stream(stream), p,
                       d_upstream, (float)((double)desc->n_rays * desc->n_fine));
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_ray_distortion_bytes(const pixie_ray_distortion_desc* desc, int64_t* scratch_bytes) {
    if (int rc = check_distortion(desc, "pixie_ray_distortion_bytes")) return rc;
    PX_REQUIRE(scratch_bytes != nullptr, "pixie_ray_distortion_bytes: scratch_bytes is NULL");
    *scratch_bytes = 4 * desc->n_rays;
    return 0;
}

extern "C" int pixie_ray_distortion_forward(const pixie_ray_distortion_desc* desc, const float* d_edges, const float* d_weights, float* d_loss,
                                            void* d_scratch, void* stream) {
    const char* who = "pixie_ray_distortion_forward";
    if (int rc = check_distortion(desc, who)) return rc;
    PX_REQUIRE(d_edges && d_weights && d_scratch, "%s: NULL argument", who);
    hipStream_t st = as_stream(stream);
    hipLaunchKernelGGL(distortion_forward_kernel, dim3((unsigned)desc->n_rays), dim3(kWave), 0, st, d_edges, d_weights, desc->n_samples,
                       (float*)d_scratch);
    PX_CHECK_HIP(hipGetLastError());
    if (d_loss == nullptr) return 0;                               // lossfun_distortion: the per-ray values in d_scratch are the output
    hipLaunchKernelGGL(loss_finalise_kernel, dim3(1), dim3(kFinaliseBlock), 0, st, (const float*)d_scratch, desc->n_rays,
                       1.0 / (double)desc->n_rays, d_loss);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_ray_distortion_backward(const pixie_ray_distortion_desc* desc, const float* d_edges, const float* d_weights,
                                             const float* d_upstream, float* d_grad_weights, void* stream) {
    const char* who = "pixie_ray_distortion_backward";
    if (int rc = check_distortion(desc, who)) return rc;
    PX_REQUIRE(d_edges && d_weights && d_upstream && d_grad_weights, "%s: NULL argument", who);
    hipLaunchKernelGGL(distortion_backward_kernel, dim3((unsigned)desc->n_rays), dim3(kWave), 0, as_stream(stream), d_edges, d_weights,
                       desc->n_samples, d_upstream, desc->per_ray, (float)desc->n_rays, d_grad_weights);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}
