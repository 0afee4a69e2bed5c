// pixie_amd/csrc/gs_optim.hip -- the 3DGS training step after the backward pass (gaussian-splatting/train.py:114-131): the Adam
// update of all parameter groups in one launch, the densification statistics in one launch, and densify_and_prune
// (scene/gaussian_model.py:353-405) as classify + scan + one synchronise + one emit launch.  Per-element arithmetic: gs_optim_math.h.
//
//   gs_adam_kernel        one lane per 16-byte chunk of the flattened index space of all groups.  Every group is padded to whole
//                         float4 chunks, so a chunk never straddles two groups; its group comes from a prefix table of at most 8
//                         entries that is compared against with constant indices (no private copy of the descriptor, so no
//                         scratch) and is wave-uniform away from group boundaries.  Four 16-byte loads and three 16-byte stores
//                         per lane; the last chunk of a group, and every chunk of a group whose pointers are not 16-byte aligned,
//                         goes element by element.
//   gs_stats_kernel       one lane per Gaussian.
//   gs_classify_kernel    one lane per Gaussian: the row's flags (gs_optim_math.h:classify) as the five scan inputs
//                         (self kept, clone kept, children kept, split, cloned).
//   hipcub ExclusiveScan  over n + 1 count tuples (the last is 0): every destination, the rank among the split, and the totals.
//   [one stream synchronise: the host reads the totals]
//   gs_emit_kernel        one 256-thread workgroup per 64 source rows.  A row's flags are the differences of its two neighbouring
//                         scan values, i.e. exactly what the classify kernel decided.  Its up to four destinations go to LDS; then
//                         every field and moment array is one pass in which consecutive lanes read consecutive floats of the 64
//                         rows (f_rest: 64 x 180 B contiguous) and write consecutive floats of each destination row.  The two
//                         computed fields of split children (scaling, xyz) are done one (row, copy) per lane afterwards.
// The compaction is stable: destinations are scan values, so each of the four output segments is in source order.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstdint>
#include <cstring>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "gs_optim_math.h"

using namespace pixie;
namespace gm = pixie::gso;

namespace {

constexpr int kBlock = 256;
constexpr int kTileRows = 64;

// ---------------------------------------------------------------------------------------------------------------- Adam
struct AdamLaunch {
    pixie_gs_adam_group group[gm::kMaxGroups];
    int64_t chunk0[gm::kMaxGroups + 1];   // first chunk of each group in the flattened index space; [n_groups] = total
    int32_t vec_ok[gm::kMaxGroups];       // all four pointers 16-byte aligned
    float w1, beta2, w2, eps;
    int32_t n_groups;
};

__global__ void __launch_bounds__(kBlock) gs_adam_kernel(const AdamLaunch L) {
    const int64_t c = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (c >= L.chunk0[gm::kMaxGroups]) return;
    // the group of this chunk: constant indices only, so the descriptor stays in scalar registers
    float* p = L.group[0].param;
    const float* g = L.group[0].grad;
    float* m = L.group[0].exp_avg;
    float* v = L.group[0].exp_avg_sq;
    int64_t count = L.group[0].count, first = 0;
    float step_size = L.group[0].step_size, bc2 = L.group[0].bias_correction2_sqrt;
    int vec = L.vec_ok[0];
#pragma unroll
    for (int k = 1; k < gm::kMaxGroups; ++k) {
        if (c >= L.chunk0[k]) {           // chunk0 is non-decreasing and padded with the total, so the last hit is the group
            p = L.group[k].param; g = L.group[k].grad; m = L.group[k].exp_avg; v = L.group[k].exp_avg_sq;
            count = L.group[k].count; first = L.chunk0[k];
            step_size = L.group[k].step_size; bc2 = L.group[k].bias_correction2_sqrt; vec = L.vec_ok[k];
        }
    }
    const int64_t base = (c - first) * 4;
    if (vec && base + 4 <= count) {
        float4 p4 = *reinterpret_cast<const float4*>(p + base);
        const float4 g4 = *reinterpret_cast<const float4*>(g + base);
        float4 m4 = *reinterpret_cast<const float4*>(m + base);
        float4 v4 = *reinterpret_cast<const float4*>(v + base);
        gm::adam_element(p4.x, g4.x, m4.x, v4.x, L.w1, L.beta2, L.w2, L.eps, step_size, bc2);
        gm::adam_element(p4.y, g4.y, m4.y, v4.y, L.w1, L.beta2, L.w2, L.eps, step_size, bc2);
        gm::adam_element(p4.z, g4.z, m4.z, v4.z, L.w1, L.beta2, L.w2, L.eps, step_size, bc2);
        gm::adam_element(p4.w, g4.w, m4.w, v4.w, L.w1, L.beta2, L.w2, L.eps, step_size, bc2);
        *reinterpret_cast<float4*>(p + base) = p4;
        *reinterpret_cast<float4*>(m + base) = m4;
        *reinterpret_cast<float4*>(v + base) = v4;
    } else {
        const int64_t end = base + 4 < count ? base + 4 : count;
        for (int64_t i = base; i < end; ++i) {
            float pe = p[i], me = m[i], ve = v[i];
            gm::adam_element(pe, g[i], me, ve, L.w1, L.beta2, L.w2, L.eps, step_size, bc2);
            p[i] = pe; m[i] = me; v[i] = ve;
        }
    }
}

// ---------------------------------------------------------------------------------------------------------------- statistics
__global__ void __launch_bounds__(kBlock)
gs_stats_kernel(const int32_t* __restrict__ radii, const float* __restrict__ vgrad, int64_t n, float* __restrict__ max_radii,
                float* __restrict__ accum, float* __restrict__ denom) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i >= n) return;
    const int32_t r = radii[i];
    if (r <= 0) return;
    max_radii[i] = fmaxf(max_radii[i], (float)r);
    accum[i] = accum[i] + gm::stats_norm2(vgrad[i * 3], vgrad[i * 3 + 1]);
    denom[i] = denom[i] + 1.0f;
}

// ---------------------------------------------------------------------------------------------------------------- densify
struct Quad {                             // running counts: rows kept as themselves, clones kept, split rows whose children are kept,
    uint32_t self, clone, child, split, made;   // split rows, clones made (kept or not)
};
struct QuadSum {
    __host__ __device__ __forceinline__ Quad operator()(const Quad& a, const Quad& b) const {
        return Quad{a.self + b.self, a.clone + b.clone, a.child + b.child, a.split + b.split, a.made + b.made};
    }
};

constexpr size_t kHeadBytes = 256;

struct Layout {
    size_t flags, offsets, scan_temp, scan_temp_bytes, total_bytes;
};

size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int make_layout(int64_t n, Layout& L) {
    L.flags = kHeadBytes;
    L.offsets = align256(L.flags + sizeof(Quad) * (size_t)(n + 1));
    L.scan_temp = align256(L.offsets + sizeof(Quad) * (size_t)(n + 1));
    L.scan_temp_bytes = 0;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveScan(nullptr, L.scan_temp_bytes, (const Quad*)nullptr, (Quad*)nullptr, QuadSum(), Quad{0, 0, 0, 0, 0},
                                                   (int)(n + 1)));
    L.total_bytes = align256(L.scan_temp + L.scan_temp_bytes + 16);
    return 0;
}

struct Thresholds {
    float max_grad, dense_thr, min_opacity, world_thr;
    int32_t has_world_thr;
};

Thresholds thresholds_of(const pixie_gs_densify_desc* d) {
    Thresholds t;
    t.max_grad = (float)d->max_grad;
    t.dense_thr = (float)(d->percent_dense * d->extent);
    t.min_opacity = (float)d->min_opacity;
    t.world_thr = (float)(0.1 * d->extent);
    t.has_world_thr = d->has_max_screen_size ? 1 : 0;
    return t;
}

__global__ void __launch_bounds__(kBlock)
gs_classify_kernel(int64_t n, const float* __restrict__ accum, const float* __restrict__ denom, const float* __restrict__ scaling,
                   const float* __restrict__ opacity, const Thresholds t, Quad* __restrict__ flags) {
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (i > n) return;
    Quad q{0, 0, 0, 0, 0};                   // the scan runs over n + 1 entries: the last is zero
    if (i < n) {
        const float s[3] = {scaling[i * 3], scaling[i * 3 + 1], scaling[i * 3 + 2]};
        const int f = gm::classify(accum[i], denom[i], s, opacity[i], t.max_grad, t.dense_thr, t.min_opacity, t.has_world_thr, t.world_thr);
        q.self = (f & gm::kKeepSelf) ? 1u : 0u;
        q.clone = (f & gm::kKeepClone) ? 1u : 0u;
        q.child = (f & gm::kKeepChildren) ? 1u : 0u;
        q.split = (f & gm::kIsSplit) ? 1u : 0u;
        q.made = (f & gm::kIsClone) ? 1u : 0u;
    }
    flags[i] = q;
}

struct EmitArgs {
    int64_t n, n_out, n_split;
    int32_t n_rest;
    const float* noise;
    const float* in_param[6];
    const float* in_m[6];
    const float* in_v[6];
    float* out_param[6];
    float* out_m[6];
    float* out_v[6];
    int32_t* source_index;
    float* accum;
    float* denom;
    float* max_radii;
};

// One pass over `rows` rows of width `w` of one array.  mode 0: the value goes to all four destinations (a copied field);
// mode 1: it goes to the row itself and its clone only (xyz and scaling: the children's are computed afterwards);
// mode 2: a moment: the row itself keeps it, every new row gets zero.  src may be null in mode 2 (no state yet: zero).
__device__ __forceinline__ void emit_pass(const float* __restrict__ src, float* __restrict__ dst, int w, int mode, int64_t row0, int rows,
                                          const int64_t (*s_dst)[4]) {
    if (w == 0) return;
    const int cnt = rows * w;
    for (int idx = threadIdx.x; idx < cnt; idx += kBlock) {
        const int r = idx / w, e = idx - r * w;
        const int64_t d0 = s_dst[r][0], d1 = s_dst[r][1], d2 = s_dst[r][2], d3 = s_dst[r][3];
        if ((d0 & d1 & d2 & d3) < 0) continue;          // all four are -1: the row leaves nothing
        const float val = src ? src[(size_t)row0 * w + idx] : 0.0f;
        const float fresh = mode == 2 ? 0.0f : val;
        if (d0 >= 0) dst[(size_t)d0 * w + e] = val;
        if (d1 >= 0) dst[(size_t)d1 * w + e] = fresh;
        if (mode != 1) {
            if (d2 >= 0) dst[(size_t)d2 * w + e] = fresh;
            if (d3 >= 0) dst[(size_t)d3 * w + e] = fresh;
        }
    }
}

__global__ void __launch_bounds__(kBlock) gs_emit_kernel(const EmitArgs A, const Quad* __restrict__ offsets) {
    __shared__ int64_t s_dst[kTileRows][4];
    __shared__ int64_t s_rank[kTileRows];
    const int tid = threadIdx.x;
    const int64_t row0 = (int64_t)blockIdx.x * kTileRows;
    const int rows = (int)(A.n - row0 < kTileRows ? A.n - row0 : kTileRows);
    const Quad total = offsets[A.n];
    if (tid < rows) {
        const int64_t i = row0 + tid;
        const Quad o0 = offsets[i], o1 = offsets[i + 1];
        int64_t d[4] = {-1, -1, -1, -1};
        if (o1.self != o0.self) d[0] = (int64_t)o0.self;
        if (o1.clone != o0.clone) d[1] = (int64_t)total.self + o0.clone;
        if (o1.child != o0.child) {
            d[2] = (int64_t)total.self + total.clone + o0.child;
            d[3] = d[2] + total.child;
        }
        const int64_t rank = o1.split != o0.split ? (int64_t)o0.split : -1;
        // the caller's sizes bound every write and every noise read
        for (int k = 0; k < 4; ++k)
            if (d[k] >= A.n_out) d[k] = -1;
        if (rank < 0 || rank >= A.n_split) d[2] = d[3] = -1;
        for (int k = 0; k < 4; ++k) {
            s_dst[tid][k] = d[k];
            if (d[k] >= 0) {
                A.source_index[d[k]] = (int32_t)i;
                A.accum[d[k]] = 0.0f;
                A.denom[d[k]] = 0.0f;
                A.max_radii[d[k]] = 0.0f;
            }
        }
        s_rank[tid] = rank;
    }
    __syncthreads();

    const auto sd = (const int64_t (*)[4])s_dst;
    // widths: xyz 3, f_dc 3, f_rest n_rest, opacity 1, scaling 3, rotation 4
    emit_pass(A.in_param[0], A.out_param[0], 3, 1, row0, rows, sd);
    emit_pass(A.in_param[1], A.out_param[1], 3, 0, row0, rows, sd);
    emit_pass(A.in_param[2], A.out_param[2], A.n_rest, 0, row0, rows, sd);
    emit_pass(A.in_param[3], A.out_param[3], 1, 0, row0, rows, sd);
    emit_pass(A.in_param[4], A.out_param[4], 3, 1, row0, rows, sd);
    emit_pass(A.in_param[5], A.out_param[5], 4, 0, row0, rows, sd);
    emit_pass(A.in_m[0], A.out_m[0], 3, 2, row0, rows, sd);
    emit_pass(A.in_m[1], A.out_m[1], 3, 2, row0, rows, sd);
    emit_pass(A.in_m[2], A.out_m[2], A.n_rest, 2, row0, rows, sd);
    emit_pass(A.in_m[3], A.out_m[3], 1, 2, row0, rows, sd);
    emit_pass(A.in_m[4], A.out_m[4], 3, 2, row0, rows, sd);
    emit_pass(A.in_m[5], A.out_m[5], 4, 2, row0, rows, sd);
    emit_pass(A.in_v[0], A.out_v[0], 3, 2, row0, rows, sd);
    emit_pass(A.in_v[1], A.out_v[1], 3, 2, row0, rows, sd);
    emit_pass(A.in_v[2], A.out_v[2], A.n_rest, 2, row0, rows, sd);
    emit_pass(A.in_v[3], A.out_v[3], 1, 2, row0, rows, sd);
    emit_pass(A.in_v[4], A.out_v[4], 3, 2, row0, rows, sd);
    emit_pass(A.in_v[5], A.out_v[5], 4, 2, row0, rows, sd);

    // the computed fields of the split children: one (row, copy) per lane
    if (tid < 2 * kTileRows) {
        const int r = tid & (kTileRows - 1), copy = tid >> 6;
        if (r < rows) {
            const int64_t d = s_dst[r][2 + copy];
            if (d >= 0) {
                const int64_t i = row0 + r;
                const float* zp = A.noise + ((size_t)copy * A.n_split + s_rank[r]) * 3;
                const float xyz[3] = {A.in_param[0][i * 3], A.in_param[0][i * 3 + 1], A.in_param[0][i * 3 + 2]};
                const float s[3] = {A.in_param[4][i * 3], A.in_param[4][i * 3 + 1], A.in_param[4][i * 3 + 2]};
                const float q[4] = {A.in_param[5][i * 4], A.in_param[5][i * 4 + 1], A.in_param[5][i * 4 + 2], A.in_param[5][i * 4 + 3]};
                const float z[3] = {zp[0], zp[1], zp[2]};
                float np[3], ns[3];
                gm::split_position(xyz, s, q, z, np);
                gm::split_scaling(s, ns);
                for (int k = 0; k < 3; ++k) {
                    A.out_param[0][d * 3 + k] = np[k];
                    A.out_param[4][d * 3 + k] = ns[k];
                }
            }
        }
    }
}

int check_densify_desc(const pixie_gs_densify_desc* d, const char* who, Layout& L) {
    PX_REQUIRE(d, "%s: null descriptor", who);
    if (!(d->max_grad > 0.0)) {
        set_error("%s: max_grad %g is not positive (the reference would then split the clones it has just made)", who, d->max_grad);
        return PIXIE_GS_DENSIFY_BAD_MAX_GRAD;
    }
    PX_REQUIRE(d->n >= 0, "%s: n %lld < 0", who, (long long)d->n);
    if (d->n > (int64_t)INT_MAX - 1) {
        set_error("%s: %lld Gaussians exceed the 2^31 - 2 one call takes", who, (long long)d->n);
        return PIXIE_GS_DENSIFY_TOO_MANY_ROWS;
    }
    if (d->n == 0) {
        set_error("%s: there is no Gaussian to densify or prune (n == 0)", who);
        return PIXIE_GS_DENSIFY_EMPTY;
    }
    PX_REQUIRE(d->n_rest >= 0 && d->n_rest <= 45 && d->n_rest % 3 == 0, "%s: n_rest %d is not 3 ((sh_degree + 1)^2 - 1) for a degree 0..3", who,
               d->n_rest);
    PX_REQUIRE(d->d_xyz_gradient_accum && d->d_denom, "%s: null statistics pointer", who);
    for (int f = 0; f < 6; ++f)
        PX_REQUIRE(d->d_param[f] || (f == 2 && d->n_rest == 0), "%s: null parameter pointer %d", who, f);
    if (make_layout(d->n, L)) return 1;
    PX_REQUIRE(d->d_workspace && d->workspace_bytes >= (int64_t)L.total_bytes,
               "%s: workspace of %lld bytes is smaller than the %lld bytes that %lld Gaussians need", who, (long long)d->workspace_bytes,
               (long long)L.total_bytes, (long long)d->n);
    PX_REQUIRE(((uintptr_t)d->d_workspace & 15) == 0, "%s: d_workspace must be 16-byte aligned", who);
    return 0;
}

}  // namespace

extern "C" {

int pixie_gs_adam_step(const pixie_gs_adam_desc* d, void* stream) {
    PX_REQUIRE(d, "pixie_gs_adam_step: null descriptor");
    PX_REQUIRE(d->n_groups >= 0 && d->n_groups <= gm::kMaxGroups, "pixie_gs_adam_step: n_groups %d outside 0..%d", d->n_groups, gm::kMaxGroups);
    AdamLaunch L;
    memset(&L, 0, sizeof L);
    L.w1 = (float)(1.0 - d->beta1);      // torch hands its kernels the double 1 - beta, rounded once
    L.beta2 = (float)d->beta2;
    L.w2 = (float)(1.0 - d->beta2);
    L.eps = (float)d->eps;
    L.n_groups = d->n_groups;
    int64_t chunks = 0;
    for (int k = 0; k < gm::kMaxGroups; ++k) {
        L.chunk0[k] = chunks;
        if (k >= d->n_groups) continue;
        const pixie_gs_adam_group& g = d->group[k];
        PX_REQUIRE(g.count >= 0, "pixie_gs_adam_step: group %d has count %lld < 0", k, (long long)g.count);
        if (g.count == 0) continue;
        PX_REQUIRE(g.param && g.grad && g.exp_avg && g.exp_avg_sq, "pixie_gs_adam_step: group %d has a null pointer", k);
        L.group[k] = g;
        L.vec_ok[k] = ((((uintptr_t)g.param | (uintptr_t)g.grad | (uintptr_t)g.exp_avg | (uintptr_t)g.exp_avg_sq) & 15) == 0) ? 1 : 0;
        chunks += (g.count + 3) / 4;
    }
    L.chunk0[gm::kMaxGroups] = chunks;
    if (chunks == 0) return 0;
    const int64_t blocks = (chunks + kBlock - 1) / kBlock;
    PX_REQUIRE(blocks <= (int64_t)INT_MAX, "pixie_gs_adam_step: %lld floats exceed one launch", (long long)(chunks * 4));
    hipLaunchKernelGGL(gs_adam_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), L);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_gs_densify_stats(const int32_t* d_radii, const float* d_viewspace_grad, int64_t n, float* d_max_radii2D,
                           float* d_xyz_gradient_accum, float* d_denom, void* stream) {
    PX_REQUIRE(n >= 0, "pixie_gs_densify_stats: n %lld < 0", (long long)n);
    if (n == 0) return 0;
    PX_REQUIRE(d_radii && d_viewspace_grad && d_max_radii2D && d_xyz_gradient_accum && d_denom, "pixie_gs_densify_stats: null pointer");
    const int64_t blocks = (n + kBlock - 1) / kBlock;
    PX_REQUIRE(blocks <= (int64_t)INT_MAX, "pixie_gs_densify_stats: %lld Gaussians exceed one launch", (long long)n);
    hipLaunchKernelGGL(gs_stats_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, as_stream(stream), d_radii, d_viewspace_grad, n, d_max_radii2D,
                       d_xyz_gradient_accum, d_denom);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int64_t pixie_gs_densify_workspace_bytes(int64_t n) {
    if (n < 0 || n > (int64_t)INT_MAX - 1) {
        set_error("pixie_gs_densify_workspace_bytes: n %lld outside [0, 2^31 - 2]", (long long)n);
        return -1;
    }
    Layout L;
    if (make_layout(n, L)) return -1;
    return (int64_t)L.total_bytes;
}

int pixie_gs_densify_plan(const pixie_gs_densify_desc* d, int64_t counts_out[4], int64_t n_split_out[1], void* stream) {
    if (counts_out) counts_out[0] = counts_out[1] = counts_out[2] = counts_out[3] = 0;
    if (n_split_out) n_split_out[0] = 0;
    Layout L;
    if (int rc = check_densify_desc(d, "pixie_gs_densify_plan", L)) return rc;
    hipStream_t st = as_stream(stream);
    char* ws = (char*)d->d_workspace;
    Quad* flags = (Quad*)(ws + L.flags);
    Quad* offsets = (Quad*)(ws + L.offsets);
    const int64_t n = d->n;
    hipLaunchKernelGGL(gs_classify_kernel, dim3((unsigned)cdiv(n + 1, kBlock)), dim3(kBlock), 0, st, n, d->d_xyz_gradient_accum, d->d_denom,
                       d->d_param[4], d->d_param[3], thresholds_of(d), flags);
    PX_CHECK_HIP(hipGetLastError());
    size_t tb = L.scan_temp_bytes;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveScan(ws + L.scan_temp, tb, (const Quad*)flags, offsets, QuadSum(), Quad{0, 0, 0, 0, 0}, (int)(n + 1), st));
    Quad total;
    PX_CHECK_HIP(hipMemcpyAsync(&total, offsets + n, sizeof total, hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipStreamSynchronize(st));          // the only one of plan + emit
    if (counts_out) {
        counts_out[0] = total.self;
        counts_out[1] = total.clone;
        counts_out[2] = 2 * (int64_t)total.child;
        // what the reference's last prune_points removes from the n - n_split originals, the clones and the 2 n_split children
        counts_out[3] = (n - total.split - total.self) + ((int64_t)total.made - total.clone) + 2 * ((int64_t)total.split - total.child);
    }
    if (n_split_out) n_split_out[0] = total.split;
    return 0;
}

int pixie_gs_densify_emit(const pixie_gs_densify_desc* d, const pixie_gs_densify_outs* o, void* stream) {
    Layout L;
    if (int rc = check_densify_desc(d, "pixie_gs_densify_emit", L)) return rc;
    PX_REQUIRE(o, "pixie_gs_densify_emit: null outputs");
    PX_REQUIRE(o->n_out >= 0 && o->n_split >= 0 && o->n_split <= d->n, "pixie_gs_densify_emit: n_out %lld or n_split %lld out of range",
               (long long)o->n_out, (long long)o->n_split);
    if (o->n_out == 0) return 0;
    PX_REQUIRE(o->d_source_index && o->d_xyz_gradient_accum && o->d_denom && o->d_max_radii2D, "pixie_gs_densify_emit: null output pointer");
    PX_REQUIRE(o->n_split == 0 || o->d_noise, "pixie_gs_densify_emit: %lld Gaussians are split and d_noise is null", (long long)o->n_split);
    EmitArgs A;
    A.n = d->n; A.n_out = o->n_out; A.n_split = o->n_split; A.n_rest = d->n_rest; A.noise = o->d_noise;
    for (int f = 0; f < 6; ++f) {
        const bool empty = f == 2 && d->n_rest == 0;
        PX_REQUIRE(empty || (o->d_param[f] && o->d_exp_avg[f] && o->d_exp_avg_sq[f]), "pixie_gs_densify_emit: null output pointer for field %d", f);
        A.in_param[f] = d->d_param[f]; A.in_m[f] = d->d_exp_avg[f]; A.in_v[f] = d->d_exp_avg_sq[f];
        A.out_param[f] = o->d_param[f]; A.out_m[f] = o->d_exp_avg[f]; A.out_v[f] = o->d_exp_avg_sq[f];
    }
    A.source_index = o->d_source_index; A.accum = o->d_xyz_gradient_accum; A.denom = o->d_denom; A.max_radii = o->d_max_radii2D;
    const Quad* offsets = (const Quad*)((const char*)d->d_workspace + L.offsets);
    hipLaunchKernelGGL(gs_emit_kernel, dim3((unsigned)cdiv(d->n, kTileRows)), dim3(kBlock), 0, as_stream(stream), A, offsets);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
