// pixie_amd/csrc/part_seg_math.h -- arithmetic of the language-query part segmentation (pixie/voxel/segmentation.py: run_clip and
// clip_part_segmentation :98-168, local_post_process_segmentation :190-226, the material fill :429-452).
//
// __host__ __device__ like occupancy_math.h: the kernels of part_segmentation.hip run it and
// tests/host_harness/part_seg_math_host.cpp runs the same functions on the CPU.  Both sides are built with -ffp-contract=off, and the
// host walks the 64 lanes of a wave and their butterfly in the kernels' order, so the dot products carry the same bits on both.
//
// Stage A: one wave per masked voxel.  The row of C float16 features is cut into C / 8 chunks of 8 (16 bytes); lane l owns chunks
// l, l + 64, l + 128, l + 192 (C <= 2048: at most kMaxChunks each).
//   half_to_float()   exact widening of the 16 stored bits
//   query_sq_part()   thread t of kNormThreads: float64 sum of q[c]^2 over c = t, t + kNormThreads, ...; tree_sum() folds the
//                     partials in a fixed tree; the norm is float32(sqrt(that)) and the staged query is q[c] / norm in float32
//   lane_dot()        float32 sum over the lane's chunks, ascending chunk, ascending element: acc = acc + f q
//   butterfly()       v += v[lane ^ 32], ^16, ... ^1 -- as __shfl_xor does it, every lane ends with the same bits
//   epilogue()        sim_j = dot_j / sqrtf(sq); label = first maximum (a NaN never wins: a zero row keeps label 0);
//                     score = 1 / sum_j expf((sim_j - sim_max) / T), j ascending
// Stage B: for every masked voxel the mode of the labels of its k nearest masked voxels, itself included, neighbours ordered by
// (integer squared offset, C-order index of the neighbour), equal counts to the smallest label.
//   kOffsets          the offsets with n <= kFastR2, sorted by (n, di, dj, dk): for a fixed centre that is the order above
//   Tally             32 labels x 8-bit counters (k <= 255 cannot overflow one, nor can the sum of the lanes' tallies)
//   fast_vote()       walks kOffsets over the int8 label grid and stops at the k-th masked voxel; false when the table runs out
//   The slow path grows a clipped cube, bisects the squared radius T by counts and takes the members at n == T in
//   C order; that part is wave code and lives in part_segmentation.hip, the host harness restates it serially with the same helpers.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define PS_HD __host__ __device__ __forceinline__
#define PS_UNROLL _Pragma("unroll")
#else
#define PS_HD inline
#define PS_UNROLL
#endif

namespace pixie {
namespace pseg {

constexpr int kMaxParts = 32;             // labels fit the tally and an int8
constexpr int kMaxChannels = 2048;
constexpr int kMaxChunks = kMaxChannels / 8 / 64;   // chunks of 8 per lane
constexpr int kMaxQueryBytes = 96 * 1024; // K C 4, the staged queries of one workgroup
constexpr int kMaxVoteK = 255;
constexpr int kNormThreads = 256;
constexpr int kFastR = 5;                 // half-width of the fast path's neighbourhood
constexpr int kFastR2 = 25;               // largest integer squared offset in kOffsets
constexpr int kMaxOffsets = 520;

struct Offset { int8_t di, dj, dk, n; };
struct OffsetTable {
    int count;
    Offset at[kMaxOffsets];
};

constexpr OffsetTable make_offsets() {
    OffsetTable t{};
    for (int n = 0; n <= kFastR2; ++n)
        for (int di = -kFastR; di <= kFastR; ++di)
            for (int dj = -kFastR; dj <= kFastR; ++dj)
                for (int dk = -kFastR; dk <= kFastR; ++dk)
                    if (di * di + dj * dj + dk * dk == n) {
                        t.at[t.count].di = (int8_t)di; t.at[t.count].dj = (int8_t)dj; t.at[t.count].dk = (int8_t)dk;
                        t.at[t.count].n = (int8_t)n;
                        ++t.count;
                    }
    return t;
}
constexpr OffsetTable kOffsets = make_offsets();
static_assert(kOffsets.count == 515, "offsets with di^2 + dj^2 + dk^2 <= 25");

// ---------------------------------------------------------------- stage A
PS_HD float half_to_float(uint16_t h) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __half2float(__ushort_as_half(h));
#else
    const uint32_t sign = (uint32_t)(h & 0x8000u) << 16;
    uint32_t exp = (h >> 10) & 0x1fu, man = h & 0x3ffu, bits;
    if (exp == 0) {
        if (man == 0) bits = sign;
        else {                                                        // subnormal: renormalise
            int e = -1;
            do { ++e; man <<= 1; } while (!(man & 0x400u));
            bits = sign | ((uint32_t)(127 - 15 - e) << 23) | ((man & 0x3ffu) << 13);
        }
    } else if (exp == 31) bits = sign | 0x7f800000u | (man << 13);
    else bits = sign | ((exp + 127 - 15) << 23) | (man << 13);
    union { uint32_t u; float f; } cv;
    cv.u = bits;
    return cv.f;
#endif
}

PS_HD double query_sq_part(const float* q, int c, int t) {
    double acc = 0.0;
    for (int e = t; e < c; e += kNormThreads) acc += (double)q[e] * (double)q[e];
    return acc;
}
// folds v[0 .. n) (n a power of two) into v[0]: v[t] += v[t + w], w = n / 2 ... 1 -- serial form of the kernels' LDS tree
template <class T>
PS_HD void tree_sum(T* v, int n) {
    for (int w = n / 2; w > 0; w >>= 1)
        for (int t = 0; t < w; ++t) v[t] += v[t + w];
}
PS_HD float norm_of(double sq) { return (float)sqrt(sq); }

// the lane's share of <f, q> (q == nullptr: of <f, f>); f holds the lane's chunks widened, chunk m at f[8 m]
PS_HD float lane_dot(const float* f, const float* q, int lane, int n_chunks) {
    float acc = 0.0f;
    PS_UNROLL
    for (int m = 0; m < kMaxChunks; ++m) {
        const int chunk = lane + 64 * m;
        if (chunk >= n_chunks) break;
        PS_UNROLL
        for (int e = 0; e < 8; ++e) {
            const float a = f[8 * m + e];
            acc = acc + a * (q ? q[8 * chunk + e] : a);
        }
    }
    return acc;
}
// host form of the wave's xor butterfly over 64 values; v[0] (every slot, on the device) holds the sum
PS_HD void butterfly(float* v) {
    for (int sft = 32; sft > 0; sft >>= 1) {
        float nxt[64];
        for (int l = 0; l < 64; ++l) nxt[l] = v[l] + v[l ^ sft];
        for (int l = 0; l < 64; ++l) v[l] = nxt[l];
    }
}

// dots[j] = <f, q_j / |q_j|>, sq = <f, f>; returns the label and writes the score
PS_HD int epilogue(const float* dots, int n_parts, float sq, float temperature, float* score) {
    const float norm = sqrtf(sq);
    int best = 0;
    float sim_max = dots[0] / norm;
    for (int j = 1; j < n_parts; ++j) {
        const float s = dots[j] / norm;
        if (s > sim_max) { sim_max = s; best = j; }
    }
    float sum = 0.0f;
    for (int j = 0; j < n_parts; ++j) sum = sum + expf((dots[j] / norm - sim_max) / temperature);
    *score = 1.0f / sum;
    return best;
}

// one row of the material grid: props[label] or [0, 0, 0, background_id]
PS_HD void material_row(const float* props, int label, float background_id, float out[4]) {
    if (label < 0) { out[0] = 0.0f; out[1] = 0.0f; out[2] = 0.0f; out[3] = background_id; return; }
    for (int e = 0; e < 4; ++e) out[e] = props[4 * label + e];
}

// ---------------------------------------------------------------- stage B
struct Tally { uint32_t w[8]; };
PS_HD void tally_clear(Tally& t) { for (int i = 0; i < 8; ++i) t.w[i] = 0u; }
PS_HD void tally_add(Tally& t, int label) {                           // no dynamic register index: eight selects
    const uint32_t one = 1u << ((label & 3) * 8);
    const int word = label >> 2;
    for (int i = 0; i < 8; ++i) t.w[i] += (i == word) ? one : 0u;
}
PS_HD int tally_mode(const Tally& t) {                                // first maximum: equal counts go to the smallest label
    int best = 0;
    uint32_t best_count = 0u;
    for (int i = 0; i < 8; ++i)
        for (int b = 0; b < 4; ++b) {
            const uint32_t c = (t.w[i] >> (8 * b)) & 0xffu;
            if (c > best_count) { best_count = c; best = 4 * i + b; }
        }
    return best;
}

struct LabelGrid {
    const int8_t* labels;                                             // (D, H, W), -1 outside the mask
    int d, h, w;
};
PS_HD int label_at(const LabelGrid& g, int i, int j, int k) {
    if ((unsigned)i >= (unsigned)g.d || (unsigned)j >= (unsigned)g.h || (unsigned)k >= (unsigned)g.w) return -1;
    return g.labels[((int64_t)i * g.h + j) * g.w + k];
}

PS_HD bool fast_vote(const LabelGrid& g, const OffsetTable* tab, int i, int j, int k, int vote_k, int* label) {
    Tally t;
    tally_clear(t);
    int seen = 0;
    for (int e = 0; e < tab->count; ++e) {
        const int l = label_at(g, i + tab->at[e].di, j + tab->at[e].dj, k + tab->at[e].dk);
        if (l < 0) continue;
        tally_add(t, l);
        if (++seen == vote_k) {
            *label = tally_mode(t);
            return true;
        }
    }
    return false;
}

PS_HD int64_t isqrt64(int64_t v) {
    int64_t r = (int64_t)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// the clipped cube of half-width r around (ci, cj, ck); item q in C order: i slowest
struct Cube {
    int i0, j0, k0, ni, nj, nk;
    int64_t items;
};
PS_HD Cube cube_of(const LabelGrid& g, int ci, int cj, int ck, int64_t r) {
    Cube c;
    const int64_t i0 = ci - r < 0 ? 0 : ci - r, j0 = cj - r < 0 ? 0 : cj - r, k0 = ck - r < 0 ? 0 : ck - r;
    const int64_t i1 = ci + r > g.d - 1 ? g.d - 1 : ci + r, j1 = cj + r > g.h - 1 ? g.h - 1 : cj + r, k1 = ck + r > g.w - 1 ? g.w - 1 : ck + r;
    c.i0 = (int)i0; c.j0 = (int)j0; c.k0 = (int)k0;
    c.ni = (int)(i1 - i0 + 1); c.nj = (int)(j1 - j0 + 1); c.nk = (int)(k1 - k0 + 1);
    c.items = (int64_t)c.ni * c.nj * c.nk;
    return c;
}
// the cube that holds every voxel with n <= T: half-width floor(sqrt(T))
PS_HD Cube cube_for(const LabelGrid& g, int ci, int cj, int ck, int64_t T) { return cube_of(g, ci, cj, ck, isqrt64(T)); }
// label of item q (-1: not masked) and its integer squared offset from the centre
PS_HD int cube_item(const LabelGrid& g, const Cube& c, int64_t q, int ci, int cj, int ck, int64_t* n) {
    const int64_t row = q / c.nk, ii = row / c.nj;
    const int k = c.k0 + (int)(q - row * c.nk), j = c.j0 + (int)(row - ii * c.nj), i = c.i0 + (int)ii;
    const int64_t di = i - ci, dj = j - cj, dk = k - ck;
    *n = di * di + dj * dj + dk * dk;
    return g.labels[((int64_t)i * g.h + j) * g.w + k];
}

}  // namespace pseg
}  // namespace pixie
