// pixie_amd/csrc/part_segmentation.hip -- material_mode=vlm's part segmentation (pixie/voxel/segmentation.py) on the device: every
// masked voxel of the CLIP feature grid is scored against K text embeddings, labelled with the best part, optionally re-labelled
// by the vote of its k nearest masked voxels, and the dense material grid is filled.  The arithmetic is part_seg_math.h; this file
// is built with -ffp-contract=off.
//
// One pixie_part_segmentation call is the chain (no stream synchronise, no host read-back; every launch is sized by the grid, work
// that depends on a count reads it on the device):
//   [memsets: the counts, the head of the scratch buffer]
//   ps_norm_kernel        one workgroup per query: float64 square sum by a fixed tree, q / float32(norm) to scratch
//   ps_list_kernel        one lane per voxel: masked voxels are appended to the work list (one integer atomic per workgroup of 1024;
//                         the order of the list does not reach the output, every voxel writes its own slot), the others get
//                         label -1 and score NaN
//   ps_row_kernel         stage A.  The normalised queries are staged once per workgroup in LDS (K C 4 <= 96 KB); one wave per
//                         work item, a fixed number of waves striding over the list.  A lane reads its 16-byte chunks of the
//                         2 C-byte row (C is a multiple of 8, so every chunk is a 16-byte load and no 8-byte tail is left), keeps
//                         them widened (the next row's loads are issued first), and forms its share of the square sum and of the K dot products; a fixed-order xor
//                         butterfly reduces each; lane 0 runs pseg::epilogue and writes label and score
//   ps_count_kernel       voxels per part from the label grid: ballots, then one integer atomic per part and workgroup (an atomic
//                         per voxel on K addresses cost more than the rest of stage A)
//   ps_vote_fast_kernel   stage B, one lane per work item: pseg::fast_vote over the sorted offset table (n <= 25, 515 offsets).
//                         A voxel whose k nearest do not fit appends its index to the slow list (one integer atomic per wave)
//   ps_vote_slow_kernel   one wave per slow voxel: doubles the half-width r of a clipped cube until the ball of radius r holds k
//                         masked voxels (or the cube is the grid), bisects the integer squared radius T > 25 by counts, tallies the
//                         labels with n < T and the first k - count(n < T) with n == T in C order by ballot prefix
//   ps_material_kernel    one lane per voxel: props[label] or [0, 0, 0, background_id], from the voted labels if stage B ran
// The output is bit-identical from run to run: no floating-point atomics, fixed reduction trees.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "part_seg_math.h"

using namespace pixie;
namespace pm = pixie::pseg;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kRowBlocks = 1536;                       // 6144 waves stride over the work list (profiles/part_segmentation_kernel_resources.txt)
constexpr int kListBlock = 1024;                       // ps_list_kernel: one atomic per 1024 voxels
constexpr int kCountBlocks = 256;
constexpr int kSlowBlocks = 1024;                      // 4096 waves stride over the slow list
constexpr size_t kHeadBytes = 256;
static_assert(kBlock == pm::kNormThreads, "ps_norm_kernel's tree");

__constant__ pm::OffsetTable d_offsets = pm::make_offsets();

struct Head {
    unsigned int n_list, n_slow;
};

struct Layout {
    size_t qn, list, slow, total_bytes;
};

size_t take(size_t& cursor, size_t bytes) {
    const size_t at = cursor;
    cursor = (cursor + bytes + 255) & ~(size_t)255;
    return at;
}

Layout make_layout(int64_t n, int parts, int channels, bool vote) {
    Layout L;
    size_t cur = kHeadBytes;
    L.qn = take(cur, 4 * (size_t)parts * (size_t)channels);
    L.list = take(cur, 4 * (size_t)n);
    L.slow = vote ? take(cur, 4 * (size_t)n) : 0;
    L.total_bytes = cur;
    return L;
}

__device__ __forceinline__ float wave_sum(float v) {
    for (int sft = 32; sft > 0; sft >>= 1) v = v + __shfl_xor(v, sft, 64);     // pseg::butterfly: the same bits in every lane
    return v;
}
__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft, 64);
    return v;
}

__global__ void __launch_bounds__(kBlock)
ps_norm_kernel(const float* __restrict__ q, int channels, float* __restrict__ qn) {
    __shared__ double s_red[kBlock];
    const float* row = q + (size_t)blockIdx.x * channels;
    s_red[threadIdx.x] = pm::query_sq_part(row, channels, (int)threadIdx.x);
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {                                 // pseg::tree_sum
        if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
        __syncthreads();
    }
    const float norm = pm::norm_of(s_red[0]);
    for (int e = threadIdx.x; e < channels; e += kBlock) qn[(size_t)blockIdx.x * channels + e] = row[e] / norm;
}

__global__ void __launch_bounds__(kListBlock)
ps_list_kernel(int64_t n, const uint8_t* __restrict__ mask, int32_t* __restrict__ list, Head* __restrict__ head,
               int8_t* __restrict__ labels, float* __restrict__ scores, int8_t* __restrict__ voted) {
    __shared__ unsigned int s_base[kListBlock / 64];
    const int64_t v = (int64_t)blockIdx.x * kListBlock + threadIdx.x;
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const bool on = v < n && mask[v] != 0;
    if (v < n && !on) {
        labels[v] = -1;
        scores[v] = NAN;
        if (voted) voted[v] = -1;
    }
    const unsigned long long bits = __ballot(on);
    if (lane == 0) s_base[wib] = (unsigned int)__popcll(bits);
    __syncthreads();
    if (threadIdx.x == 0) {                                                    // one atomic per workgroup: the waves' counts -> their bases
        unsigned int total = 0;
        for (int w = 0; w < kListBlock / 64; ++w) total += s_base[w];
        unsigned int base = total ? atomicAdd(&head->n_list, total) : 0u;
        for (int w = 0; w < kListBlock / 64; ++w) {
            const unsigned int c = s_base[w];
            s_base[w] = base;
            base += c;
        }
    }
    __syncthreads();
    if (on) list[s_base[wib] + __popcll(bits & ((1ull << lane) - 1ull))] = (int32_t)v;   // at most one entry per voxel: the list holds n
}

// voxels per part: a ballot per part and 64 voxels, lane j keeps part j's count; one integer atomic per part and workgroup
__global__ void __launch_bounds__(kBlock)
ps_count_kernel(int64_t n, const int8_t* __restrict__ labels, int parts, int64_t* __restrict__ counts) {
    __shared__ unsigned int s_hist[pm::kMaxParts];
    const int lane = threadIdx.x & 63;
    if (threadIdx.x < pm::kMaxParts) s_hist[threadIdx.x] = 0u;
    __syncthreads();
    unsigned int mine = 0;
    const int64_t rounds = (n + (int64_t)kCountBlocks * kBlock - 1) / ((int64_t)kCountBlocks * kBlock);
    for (int64_t it = 0; it < rounds; ++it) {                                  // every lane of a wave takes every round
        const int64_t v = (it * kCountBlocks + blockIdx.x) * kBlock + threadIdx.x;
        const int l = v < n ? labels[v] : -1;
        if (!__ballot(l >= 0)) continue;                                       // wave-uniform
        for (int j = 0; j < parts; ++j) {
            const unsigned long long b = __ballot(l == j);
            if (lane == j) mine += (unsigned int)__popcll(b);
        }
    }
    if (lane < parts && mine) atomicAdd(&s_hist[lane], mine);
    __syncthreads();
    if ((int)threadIdx.x < parts && s_hist[threadIdx.x]) atomicAdd((unsigned long long*)(counts + threadIdx.x), (unsigned long long)s_hist[threadIdx.x]);
}

extern __shared__ __align__(16) float s_queries[];

__global__ void __launch_bounds__(kBlock)
ps_row_kernel(const uint16_t* __restrict__ features, const float* __restrict__ qn, const int32_t* __restrict__ list,
              const Head* __restrict__ head, int channels, int parts, float temperature, int8_t* __restrict__ labels,
              float* __restrict__ scores, int64_t* __restrict__ counts) {
    const int total = parts * channels;                                        // a multiple of 8
    // the waves' dot products follow the queries in the dynamic region: the 160 KB attribute leaves no room for static LDS
    float* dots = s_queries + total + (threadIdx.x >> 6) * pm::kMaxParts;
    for (int e = 4 * (int)threadIdx.x; e < total; e += 4 * kBlock)
        *reinterpret_cast<float4*>(s_queries + e) = *reinterpret_cast<const float4*>(qn + e);
    __syncthreads();
    const int lane = threadIdx.x & 63, wib = threadIdx.x >> 6;
    const unsigned int wave = blockIdx.x * kWaves + wib;
    const unsigned int n_list = head->n_list;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[pm::kMaxParts] = (int64_t)n_list;
    const int n_chunks = channels >> 3;
    // the lane's 16-byte chunks of one row; a row is in flight while the previous one is reduced
    auto load_row = [&](int64_t v, uint4 (&raw)[pm::kMaxChunks]) {
        const uint4* row = reinterpret_cast<const uint4*>(features + (size_t)v * channels);
#pragma unroll
        for (int m = 0; m < pm::kMaxChunks; ++m) {
            const int chunk = lane + 64 * m;
            raw[m] = make_uint4(0u, 0u, 0u, 0u);
            if (chunk < n_chunks) raw[m] = row[chunk];
        }
    };
    const unsigned int stride = gridDim.x * kWaves;
    uint4 raw[pm::kMaxChunks];
    int64_t v = 0;
    if (wave < n_list) {
        v = list[wave];
        load_row(v, raw);
    }
    for (unsigned int item = wave; item < n_list; item += stride) {            // wave-uniform
        float f[8 * pm::kMaxChunks];
#pragma unroll
        for (int m = 0; m < pm::kMaxChunks; ++m) {
            const unsigned int w4[4] = {raw[m].x, raw[m].y, raw[m].z, raw[m].w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                f[8 * m + 2 * e] = pm::half_to_float((uint16_t)(w4[e] & 0xffffu));
                f[8 * m + 2 * e + 1] = pm::half_to_float((uint16_t)(w4[e] >> 16));
            }
        }
        const int64_t v_now = v;
        if (item + stride < n_list) {                                          // n_list + stride < 2^32
            v = list[item + stride];
            load_row(v, raw);
        }
        const float sq = wave_sum(pm::lane_dot(f, nullptr, lane, n_chunks));
        for (int j = 0; j < parts; ++j) {
            const float d = wave_sum(pm::lane_dot(f, s_queries + (size_t)j * channels, lane, n_chunks));
            if (lane == 0) dots[j] = d;
        }
        if (lane == 0) {                                                       // reads back its own writes
            float score;
            const int label = pm::epilogue(dots, parts, sq, temperature, &score);
            labels[v_now] = (int8_t)label;
            scores[v_now] = score;
        }
    }
}

__device__ __forceinline__ void coords_of(const pm::LabelGrid& g, int64_t v, int& ci, int& cj, int& ck) {
    ck = (int)(v % g.w);
    cj = (int)((v / g.w) % g.h);
    ci = (int)(v / ((int64_t)g.w * g.h));
}
__device__ __forceinline__ int kprime_of(int vote_k, const Head* head) {
    return head->n_list < (unsigned int)vote_k ? (int)head->n_list : vote_k;
}

__global__ void __launch_bounds__(kBlock)
ps_vote_fast_kernel(pm::LabelGrid g, const int32_t* __restrict__ list, Head* __restrict__ head, int vote_k, int8_t* __restrict__ voted,
                    int32_t* __restrict__ slow) {
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    bool to_slow = false;
    int64_t v = 0;
    if (t < (int64_t)head->n_list) {
        v = list[t];
        int ci, cj, ck, label = 0;
        coords_of(g, v, ci, cj, ck);
        to_slow = !pm::fast_vote(g, &d_offsets, ci, cj, ck, kprime_of(vote_k, head), &label);
        voted[v] = (int8_t)label;                                              // 0 for now if the slow kernel takes it
    }
    const unsigned long long bits = __ballot(to_slow);                         // one atomic per wave, as on a plate every lane appends
    if (!bits) return;                                                         // wave-uniform
    unsigned int base = 0;
    if (lane == 0) base = atomicAdd(&head->n_slow, (unsigned int)__popcll(bits));
    base = __shfl(base, 0, 64);
    if (to_slow) slow[base + __popcll(bits & ((1ull << lane) - 1ull))] = (int32_t)v;   // at most one entry per voxel: the list holds n
}

// masked voxels of the cube with n <= T, for the whole wave
__device__ __forceinline__ int64_t cube_count_le(const pm::LabelGrid& g, const pm::Cube& c, int ci, int cj, int ck, int64_t T, int lane) {
    int64_t cnt = 0;
    for (int64_t q = lane; q < c.items; q += 64) {
        int64_t n;
        const int l = pm::cube_item(g, c, q, ci, cj, ck, &n);
        cnt += (l >= 0 && n <= T) ? 1 : 0;
    }
    return wave_sum(cnt);
}

__global__ void __launch_bounds__(kBlock)
ps_vote_slow_kernel(pm::LabelGrid g, const int32_t* __restrict__ slow, const Head* __restrict__ head, int vote_k,
                    int8_t* __restrict__ voted, int64_t* __restrict__ counts) {
    const int lane = threadIdx.x & 63;
    const unsigned int wave = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const unsigned int n_slow = head->n_slow;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[pm::kMaxParts + 1] = (int64_t)n_slow;
    const int kprime = kprime_of(vote_k, head);
    const int reach = max(g.d, max(g.h, g.w));
    for (unsigned int e = wave; e < n_slow; e += kSlowBlocks * kWaves) {       // wave-uniform
        const int64_t v = slow[e];
        int ci, cj, ck;
        coords_of(g, v, ci, cj, ck);
        // smallest doubled r whose ball holds k' masked voxels; r >= reach: the cube is the whole grid, which holds n_list >= k'
        int64_t r = pm::kFastR + 1;
        int64_t lo = pm::kFastR2 + 1, hi;                                      // the answer T lies in [lo, hi]: the table held too few
        for (;;) {                                                             // at most log2(reach) + 1 rounds
            if (r >= reach) {
                const int64_t a = max(ci, g.d - 1 - ci), b = max(cj, g.h - 1 - cj), cc = max(ck, g.w - 1 - ck);
                hi = a * a + b * b + cc * cc;
                break;
            }
            hi = r * r;
            if (cube_count_le(g, pm::cube_of(g, ci, cj, ck, r), ci, cj, ck, hi, lane) >= kprime) break;
            lo = hi + 1;                                                       // the ball of radius r holds too few
            r *= 2;
        }
        while (lo < hi) {                                                      // smallest T with count(n <= T) >= k': at most 64 rounds
            const int64_t mid = lo + (hi - lo) / 2;
            if (cube_count_le(g, pm::cube_for(g, ci, cj, ck, mid), ci, cj, ck, mid, lane) >= kprime) hi = mid; else lo = mid + 1;
        }
        const int64_t T = lo;
        const int64_t below = T > 0 ? cube_count_le(g, pm::cube_for(g, ci, cj, ck, T - 1), ci, cj, ck, T - 1, lane) : 0;
        int64_t need = kprime - below;                                         // members of the last shell to take, in C order
        pm::Tally tally;
        pm::tally_clear(tally);
        const pm::Cube c = pm::cube_for(g, ci, cj, ck, T);
        const int64_t rounds = (c.items + 63) / 64;
        for (int64_t it = 0; it < rounds; ++it) {
            const int64_t q = it * 64 + lane;
            int l = -1;
            bool tie = false;
            if (q < c.items) {
                int64_t n;
                l = pm::cube_item(g, c, q, ci, cj, ck, &n);
                if (l >= 0 && n < T) pm::tally_add(tally, l);
                tie = l >= 0 && n == T;
            }
            const unsigned long long ties = __ballot(tie);
            if (!ties) continue;                                               // wave-uniform
            const int64_t rank = __popcll(ties & ((1ull << lane) - 1ull));
            if (tie && rank < need) pm::tally_add(tally, l);
            need -= __popcll(ties);
        }
        // at most k' <= 255 members in all: the byte counters of the 64 tallies add without a carry
        for (int i = 0; i < 8; ++i)
            for (int sft = 32; sft > 0; sft >>= 1) tally.w[i] += __shfl_xor(tally.w[i], sft, 64);
        if (lane == 0) voted[v] = (int8_t)pm::tally_mode(tally);
    }
}

__global__ void __launch_bounds__(kBlock)
ps_material_kernel(int64_t n, const int8_t* __restrict__ labels, const float* __restrict__ props, int parts, float background_id,
                   float4* __restrict__ material) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    const int l = labels[v];
    float row[4];
    pm::material_row(props, l < parts ? l : -1, background_id, row);
    material[v] = make_float4(row[0], row[1], row[2], row[3]);
}

int check_shape(const pixie_part_seg_desc* desc, int64_t& n, const char* who) {
    PX_REQUIRE(desc, "%s: null descriptor", who);
    PX_REQUIRE(desc->d >= 1 && desc->h >= 1 && desc->w >= 1, "%s: grid %d x %d x %d has a dimension < 1", who, desc->d, desc->h, desc->w);
    n = (int64_t)desc->d * desc->h * desc->w;
    PX_REQUIRE(n <= (int64_t)INT32_MAX - kBlock, "%s: grid %d x %d x %d exceeds the 2^31 voxels one call takes", who, desc->d, desc->h, desc->w);
    PX_REQUIRE(desc->n_parts >= 1 && desc->n_parts <= pm::kMaxParts, "%s: %d parts, 1 to %d are supported", who, desc->n_parts, pm::kMaxParts);
    PX_REQUIRE(desc->channels >= 8 && desc->channels <= pm::kMaxChannels && desc->channels % 8 == 0,
               "%s: %d channels, a multiple of 8 up to %d is supported", who, desc->channels, pm::kMaxChannels);
    PX_REQUIRE((int64_t)desc->n_parts * desc->channels * 4 <= pm::kMaxQueryBytes, "%s: %d parts x %d channels exceed the %d bytes of staged queries",
               who, desc->n_parts, desc->channels, pm::kMaxQueryBytes);
    PX_REQUIRE(desc->vote_k >= 0 && desc->vote_k <= pm::kMaxVoteK, "%s: vote_k %d, 0 (no vote) to %d are supported", who, desc->vote_k, pm::kMaxVoteK);
    return 0;
}

}  // namespace

extern "C" {

int64_t pixie_part_seg_scratch_bytes(const pixie_part_seg_desc* desc) {
    int64_t n;
    if (check_shape(desc, n, "pixie_part_seg_scratch_bytes")) return -1;
    return (int64_t)make_layout(n, desc->n_parts, desc->channels, desc->vote_k > 0).total_bytes;
}

int pixie_part_material_grid(const int8_t* d_labels, const float* d_props, int n_parts, int64_t n_voxels, float background_id,
                             float* d_material, void* stream) {
    PX_REQUIRE(d_labels && d_props && d_material, "pixie_part_material_grid: null pointer");
    PX_REQUIRE(n_parts >= 1 && n_parts <= pm::kMaxParts, "pixie_part_material_grid: %d parts, 1 to %d are supported", n_parts, pm::kMaxParts);
    PX_REQUIRE(n_voxels >= 1 && n_voxels <= (int64_t)INT32_MAX - kBlock, "pixie_part_material_grid: %lld voxels", (long long)n_voxels);
    PX_REQUIRE(((uintptr_t)d_material & 15) == 0, "pixie_part_material_grid: d_material must be 16-byte aligned");
    hipLaunchKernelGGL(ps_material_kernel, dim3((unsigned)cdiv(n_voxels, kBlock)), dim3(kBlock), 0, as_stream(stream), n_voxels, d_labels,
                       d_props, n_parts, background_id, (float4*)d_material);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_part_segmentation(const pixie_part_seg_desc* desc, int8_t* d_labels, float* d_scores, int8_t* d_voted, float* d_material,
                            int64_t* d_counts, void* d_scratch, void* stream) {
    int64_t n;
    if (check_shape(desc, n, "pixie_part_segmentation")) return 1;
    PX_REQUIRE(desc->d_features && desc->d_mask && desc->d_queries, "pixie_part_segmentation: null pointer (d_features, d_mask and d_queries are required)");
    PX_REQUIRE(d_labels && d_scores && d_counts && d_scratch, "pixie_part_segmentation: null pointer (d_labels, d_scores, d_counts and d_scratch are required)");
    PX_REQUIRE(((uintptr_t)desc->d_features & 15) == 0 && ((uintptr_t)d_scratch & 15) == 0,
               "pixie_part_segmentation: d_features and d_scratch must be 16-byte aligned");
    PX_REQUIRE((desc->vote_k > 0) == (d_voted != nullptr), "pixie_part_segmentation: d_voted goes with vote_k > 0");
    PX_REQUIRE((desc->d_props != nullptr) == (d_material != nullptr), "pixie_part_segmentation: d_material goes with d_props");
    PX_REQUIRE(((uintptr_t)d_material & 15) == 0, "pixie_part_segmentation: d_material must be 16-byte aligned");
    PX_REQUIRE(desc->temperature > 0.0f && std::isfinite(desc->temperature), "pixie_part_segmentation: temperature %g is not a positive number",
               (double)desc->temperature);

    hipStream_t st = as_stream(stream);
    const int parts = desc->n_parts, channels = desc->channels;
    const Layout L = make_layout(n, parts, channels, desc->vote_k > 0);
    char* ws = (char*)d_scratch;
    Head* head = (Head*)ws;
    float* qn = (float*)(ws + L.qn);
    int32_t* list = (int32_t*)(ws + L.list);
    int32_t* slow = (int32_t*)(ws + L.slow);
    const dim3 grid((unsigned)cdiv(n, kBlock)), block(kBlock);
    const size_t lds = 4 * ((size_t)parts * (size_t)channels + (size_t)kWaves * pm::kMaxParts);
    PX_CHECK_HIP(allow_max_dynamic_lds((const void*)ps_row_kernel));

    PX_CHECK_HIP(hipMemsetAsync(d_counts, 0, PIXIE_PART_SEG_COUNTS * sizeof(int64_t), st));
    PX_CHECK_HIP(hipMemsetAsync(head, 0, kHeadBytes, st));
    hipLaunchKernelGGL(ps_norm_kernel, dim3(parts), block, 0, st, desc->d_queries, channels, qn);
    hipLaunchKernelGGL(ps_list_kernel, dim3((unsigned)cdiv(n, kListBlock)), dim3(kListBlock), 0, st, n, desc->d_mask, list, head, d_labels, d_scores,
                       d_voted);
    PX_CHECK_HIP(hipGetLastError());
    const unsigned row_blocks = (unsigned)(cdiv(n, kWaves) < kRowBlocks ? cdiv(n, kWaves) : kRowBlocks);
    hipLaunchKernelGGL(ps_row_kernel, dim3(row_blocks), block, lds, st, (const uint16_t*)desc->d_features, qn, list, head, channels, parts,
                       desc->temperature, d_labels, d_scores, d_counts);
    hipLaunchKernelGGL(ps_count_kernel, dim3(kCountBlocks), block, 0, st, n, d_labels, parts, d_counts);
    PX_CHECK_HIP(hipGetLastError());
    if (desc->vote_k > 0) {
        const pm::LabelGrid g{d_labels, desc->d, desc->h, desc->w};
        hipLaunchKernelGGL(ps_vote_fast_kernel, grid, block, 0, st, g, list, head, desc->vote_k, d_voted, slow);
        hipLaunchKernelGGL(ps_vote_slow_kernel, dim3(kSlowBlocks), block, 0, st, g, slow, head, desc->vote_k, d_voted, d_counts);
        PX_CHECK_HIP(hipGetLastError());
    }
    if (d_material) {
        hipLaunchKernelGGL(ps_material_kernel, grid, block, 0, st, n, d_voted ? d_voted : d_labels, desc->d_props, parts, desc->background_id,
                           (float4*)d_material);
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
