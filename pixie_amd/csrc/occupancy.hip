// pixie_amd/csrc/occupancy.hip -- the occupancy mask of pixie/voxel/voxelize.py:_create_occupancy_mask on the device: density and
// gray thresholds, statistical outlier removal and floating-cluster removal (Open3D's remove_statistical_outlier and cluster_dbscan,
// restated on the voxel lattice).  The arithmetic is occupancy_math.h; this file is built with -ffp-contract=off.
//
// One pixie_occupancy_mask call is the chain (no stream synchronise, no host read-back; every launch is sized by the grid, work
// that depends on a count reads it on the device):
//   [memsets: the count record, the head of the scratch buffer, the cluster sizes]
//   occ_classify_kernel   one lane per voxel of the W-padded grid, a wave per 64-bit word: ballot -> candidate bit grid, counts
//   occ_fast_kernel       stage B, one lane per voxel: occ::fast_mean over the sorted offset table (n <= 9, 123 offsets).  A voxel
//                         whose k' nearest do not fit appends its index to the slow list (integer atomic on the list length; the
//                         order of the list does not reach the output, every voxel writes its own slot)
//   occ_slow_kernel       one wave per slow voxel, a fixed number of waves striding over the list: doubles the half-width r of a
//                         clipped cube until the ball of radius r holds k' candidates (or the cube is the grid), bisects the integer
//                         squared radius T (each probe scans only the cube of half-width floor(sqrt(T))), sums the distances below
//                         T and completes with the first ties in scan order
//   occ_reduce_kernel x2  cloud_mean, then the squared deviations: kReduceBlocks partial sums in a fixed order, folded by the last
//   occ_finish_kernel x2  stage of each; no floating-point atomics
//   occ_keep_kernel       m > 0 && m < cloud_mean + std_ratio std -> survivor bit grid
//   occ_core_kernel       stage C: open ball of eps around every survivor holds >= min_points survivors -> core bit grid, parent = self
//   occ_union_kernel      every core voxel is united with the core voxels of lower index in its ball (lock-free union-find, links go
//                         from the higher to the lower index, so a component's root is its lowest voxel index in C order)
//   occ_flatten_kernel    parent = root for every core voxel
//   occ_label_kernel      root of every survivor (border voxels: the lowest root among the core voxels in reach, -1: noise), cluster
//                         sizes and the number of clusters (integer atomics)
//   occ_best_kernel       the largest cluster, first maximum: atomicMax of (size << 32 | ~root)
//   occ_mask_kernel       the keep rule -> uint8 mask, count
// The output is bit-identical from run to run.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "occupancy_math.h"

using namespace pixie;
namespace om = pixie::occ;

namespace {

constexpr int kBlock = 256;
constexpr int kWaves = kBlock / 64;
constexpr int kReduceBlocks = 256;
constexpr int kSlowBlocks = 1024;                      // 4096 waves stride over the slow list
constexpr size_t kHeadBytes = 256;

__constant__ om::OffsetTable d_offsets = om::make_offsets();

struct Head {
    double sum_m, mean, sum_dev, std_dev, threshold;
    unsigned long long best;                           // (size << 32) | (0xffffffff - root)
    unsigned int n_slow;
};

struct Shape {
    int d, h, w, wpc;
    int64_t n;                                         // d h w
    int64_t n_words;                                   // d h wpc
};

struct Layout {
    size_t cand, surv, core, m, slow, parent, root, sizes, partials, total_bytes;
};

size_t take(size_t& cursor, size_t bytes) {
    const size_t at = cursor;
    cursor = (cursor + bytes + 255) & ~(size_t)255;
    return at;
}

Layout make_layout(const Shape& s, bool with_m) {
    Layout L;
    size_t cur = kHeadBytes;
    L.cand = take(cur, 8 * (size_t)s.n_words);
    L.surv = take(cur, 8 * (size_t)s.n_words);
    L.core = take(cur, 8 * (size_t)s.n_words);
    L.slow = take(cur, 4 * (size_t)s.n);
    L.parent = take(cur, 4 * (size_t)s.n);
    L.root = take(cur, 4 * (size_t)s.n);
    L.sizes = take(cur, 4 * (size_t)s.n);
    L.partials = take(cur, 8 * (size_t)kReduceBlocks);
    L.m = with_m ? take(cur, 8 * (size_t)s.n) : 0;     // the mean distances, unless the caller keeps them
    L.total_bytes = cur;
    return L;
}

// lane -> voxel of the padded grid: 64 consecutive lanes are the 64 bits of one word
struct Where {
    int64_t word;                                      // word index, wave-uniform
    int i, j, k;
    int64_t v;                                         // C-order voxel index, valid only if inside
    bool inside;
};
__device__ __forceinline__ Where where(const Shape& s) {
    Where p;
    const int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    p.word = t >> 6;
    const int64_t col = p.word / s.wpc;
    p.k = (int)(p.word - col * s.wpc) * 64 + (int)(t & 63);
    p.i = (int)(col / s.h);
    p.j = (int)(col - (int64_t)p.i * s.h);
    p.inside = p.word < s.n_words && p.k < s.w;
    p.v = col * s.w + p.k;
    return p;
}
__device__ __forceinline__ bool bit_of(const uint64_t* words, const Where& p) {
    return p.inside && ((words[p.word] >> (p.k & 63)) & 1ull);
}
__device__ __forceinline__ void wave_count(bool flag, int64_t* counter) {
    const unsigned long long b = __ballot(flag);
    if ((threadIdx.x & 63) == 0 && b) atomicAdd((unsigned long long*)counter, (unsigned long long)__popcll(b));
}

template <typename T>
__global__ void __launch_bounds__(kBlock)
occ_classify_kernel(Shape s, const T* __restrict__ alphas, const T* __restrict__ rgb, float alpha_thr, float gray_thr,
                    uint64_t* __restrict__ cand, int64_t* __restrict__ counts) {
    const Where p = where(s);
    bool dense = false, keep = false;
    if (p.inside) {
        const float a = (float)alphas[p.v];
        const float r = (float)rgb[3 * p.v], g = (float)rgb[3 * p.v + 1], b = (float)rgb[3 * p.v + 2];
        keep = om::classify(a, r, g, b, alpha_thr, gray_thr, &dense);
    }
    const unsigned long long bits = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && p.word < s.n_words) cand[p.word] = bits;
    wave_count(dense, counts + 0);
    wave_count(keep, counts + 1);
}

__device__ __forceinline__ int kprime_of(int nb_neighbors, const int64_t* counts) {
    const int64_t m = counts[1];
    return m < nb_neighbors ? (int)m : nb_neighbors;
}

__global__ void __launch_bounds__(kBlock)
occ_fast_kernel(Shape s, const uint64_t* __restrict__ cand, const float* __restrict__ ax, const float* __restrict__ ay,
                const float* __restrict__ az, int nb_neighbors, const int64_t* __restrict__ counts, double* __restrict__ m,
                int32_t* __restrict__ slow, Head* __restrict__ head) {
    const Where p = where(s);
    if (!p.inside) return;
    if (!bit_of(cand, p)) { m[p.v] = NAN; return; }
    const om::Grid g{cand, s.d, s.h, s.w, s.wpc};
    double mean = 0.0;
    if (om::fast_mean(g, &d_offsets, ax, ay, az, p.i, p.j, p.k, kprime_of(nb_neighbors, counts), &mean)) {
        m[p.v] = mean;
    } else {
        m[p.v] = 0.0;                                             // the slow kernel overwrites it
        slow[atomicAdd(&head->n_slow, 1u)] = (int32_t)p.v;       // at most one entry per voxel: the list holds n
    }
}

__device__ __forceinline__ int64_t wave_sum(int64_t v) {
    for (int sft = 32; sft > 0; sft >>= 1) v += __shfl_xor(v, sft, 64);
    return v;
}

// the clipped cube of half-width r around (ci, cj, ck), as rows of words; items < 2^25 (the grid's words)
struct Cube {
    int i0, j0, w0, ni, nj, nw;
    unsigned int items;
};
__device__ __forceinline__ Cube cube_of(const Shape& s, int ci, int cj, int ck, int r) {
    Cube c;
    c.i0 = max(ci - r, 0); c.j0 = max(cj - r, 0);
    const int i1 = min(ci + r, s.d - 1), j1 = min(cj + r, s.h - 1);
    c.w0 = max(ck - r, 0) >> 6;
    const int w1 = min(ck + r, s.w - 1) >> 6;
    c.ni = i1 - c.i0 + 1; c.nj = j1 - c.j0 + 1; c.nw = w1 - c.w0 + 1;
    c.items = (unsigned int)c.ni * (unsigned int)c.nj * (unsigned int)c.nw;
    return c;
}
// item q of a cube, in scan order: rows (i, then j), then the row's words
__device__ __forceinline__ void cube_item(const Cube& c, unsigned int q, int& i2, int& j2, int& wi) {
    const unsigned int row = q / (unsigned int)c.nw, ii = row / (unsigned int)c.nj;
    wi = (int)(q - row * (unsigned int)c.nw);
    j2 = c.j0 + (int)(row - ii * (unsigned int)c.nj);
    i2 = c.i0 + (int)ii;
}
// the cube that holds every voxel with n <= T: half-width floor(sqrt(T))
__device__ __forceinline__ Cube cube_for(const Shape& s, int ci, int cj, int ck, int64_t T) {
    const int64_t r = om::isqrt64(T);
    return cube_of(s, ci, cj, ck, r > INT32_MAX / 2 ? INT32_MAX / 2 : (int)r);
}

// candidates of the cube with n <= T, for the whole wave.  Rows partly outside [ck - r, ck + r] are read whole: for T <= r^2 their
// surplus bits fail n <= T anyway, and when the cube is the grid there is no surplus.
__device__ __forceinline__ int64_t cube_count_le(const Shape& s, const uint64_t* cand, const Cube& c, int ci, int cj, int ck, int64_t T,
                                                 int lane) {
    int cnt = 0;                                                                  // a cube holds fewer than 2^31 voxels
    for (unsigned int q = lane; q < c.items; q += 64) {
        int i2, j2, wi;
        cube_item(c, q, i2, j2, wi);
        const int64_t di = i2 - ci, dj = j2 - cj;
        const uint64_t word = cand[((size_t)i2 * s.h + j2) * s.wpc + c.w0 + wi];
        cnt += om::word_count_le(word, (c.w0 + wi) * 64, ck, di * di + dj * dj, T);
    }
    return wave_sum((int64_t)cnt);
}

__global__ void __launch_bounds__(kBlock)
occ_slow_kernel(Shape s, const uint64_t* __restrict__ cand, const float* __restrict__ ax, const float* __restrict__ ay,
                const float* __restrict__ az, int nb_neighbors, int64_t* __restrict__ counts, double* __restrict__ m,
                const int32_t* __restrict__ slow, const Head* __restrict__ head) {
    const int lane = threadIdx.x & 63;
    const int wave = blockIdx.x * kWaves + (threadIdx.x >> 6);
    const unsigned int n_slow = head->n_slow;
    if (blockIdx.x == 0 && threadIdx.x == 0) counts[4] = (int64_t)n_slow;
    const int kprime = kprime_of(nb_neighbors, counts);
    const int reach = max(s.d, max(s.h, s.w));
    for (unsigned int e = wave; e < n_slow; e += kSlowBlocks * kWaves) {          // wave-uniform
        const int64_t v = slow[e];
        const int ck = (int)(v % s.w), cj = (int)((v / s.w) % s.h), ci = (int)(v / ((int64_t)s.w * s.h));
        // smallest doubled r whose ball holds k' candidates; r >= reach: the cube is the whole grid, which holds M >= k'
        int r = om::kFastR + 1;
        int64_t lo = 0, hi;                                                       // the answer T lies in [lo, hi]
        for (;;) {                                                                // at most log2(reach) + 1 rounds
            if (r >= reach) {
                const int64_t a = max(ci, s.d - 1 - ci), b = max(cj, s.h - 1 - cj), cc = max(ck, s.w - 1 - ck);
                hi = a * a + b * b + cc * cc;
                break;
            }
            hi = (int64_t)r * r;
            if (cube_count_le(s, cand, cube_of(s, ci, cj, ck, r), ci, cj, ck, hi, lane) >= kprime) break;
            lo = hi + 1;                                                          // the ball of radius r holds too few
            r *= 2;
        }
        while (lo < hi) {                                                         // smallest T with count(n <= T) >= k': at most 64 rounds
            const int64_t mid = lo + (hi - lo) / 2;
            if (cube_count_le(s, cand, cube_for(s, ci, cj, ck, mid), ci, cj, ck, mid, lane) >= kprime) hi = mid; else lo = mid + 1;
        }
        const int64_t T = lo;
        const int64_t below = T > 0 ? cube_count_le(s, cand, cube_for(s, ci, cj, ck, T - 1), ci, cj, ck, T - 1, lane) : 0;
        int64_t need = kprime - below;                                            // ties to take, in scan order
        double sum = 0.0;
        const Cube c = cube_for(s, ci, cj, ck, T);
        const unsigned int rounds = (c.items + 63u) / 64u;
        for (unsigned int it = 0; it < rounds; ++it) {
            const unsigned int q = it * 64u + lane;
            uint64_t ties = 0ull;
            int i2 = 0, j2 = 0, k0 = 0;
            if (q < c.items) {
                int wi;
                cube_item(c, q, i2, j2, wi);
                k0 = (c.w0 + wi) * 64;
                const int64_t di = i2 - ci, dj = j2 - cj;
                const uint64_t word = cand[((size_t)i2 * s.h + j2) * s.wpc + c.w0 + wi];
                om::word_sum_lt(word, k0, ax, ay, az, ci, cj, ck, i2, j2, di * di + dj * dj, T, &sum, &ties);
            }
            const int mine = __popcll(ties);
            if (!__any(mine)) continue;                                           // wave-uniform
            int before = mine;                                                    // inclusive prefix over the lanes
            for (int sft = 1; sft < 64; sft <<= 1) {
                const int up = __shfl_up(before, sft, 64);
                if (lane >= sft) before += up;
            }
            const int total = __shfl(before, 63, 64);
            int64_t rank = before - mine;
            while (ties) {
                const int b = __builtin_ctzll(ties);
                ties &= ties - 1;
                if (rank < need) sum += sqrt(om::dist2_axes(ax, ay, az, ci, cj, ck, i2, j2, k0 + b));
                ++rank;
            }
            need -= total;
        }
        for (int sft = 32; sft > 0; sft >>= 1) sum += __shfl_xor(sum, sft, 64);   // a fixed tree: the same bits in every lane
        if (lane == 0) m[v] = sum / (double)kprime;
    }
}

// mode 0: sum of m over the candidates; mode 1: sum of (m - mean)^2.  Fixed grid, fixed strides, fixed tree: one order of additions.
template <int kMode>
__global__ void __launch_bounds__(kBlock)
occ_reduce_kernel(int64_t n, const double* __restrict__ m, const Head* __restrict__ head, double* __restrict__ partials) {
    __shared__ double s_red[kBlock];
    const double mean = head->mean;
    double acc = 0.0;
    for (int64_t t = (int64_t)blockIdx.x * kBlock + threadIdx.x; t < n; t += (int64_t)kReduceBlocks * kBlock) {
        const double x = m[t];
        if (x != x) continue;                                                     // NaN: not a candidate
        acc += kMode == 0 ? x : (x - mean) * (x - mean);
    }
    s_red[threadIdx.x] = acc;
    __syncthreads();
    for (int w = kBlock / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) partials[blockIdx.x] = s_red[0];
}

template <int kMode>
__global__ void __launch_bounds__(kReduceBlocks)
occ_finish_kernel(const double* __restrict__ partials, const int64_t* __restrict__ counts, double std_ratio, Head* __restrict__ head,
                  double* __restrict__ stats) {
    __shared__ double s_red[kReduceBlocks];
    s_red[threadIdx.x] = partials[threadIdx.x];
    __syncthreads();
    for (int w = kReduceBlocks / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) s_red[threadIdx.x] += s_red[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x != 0) return;
    const double big_m = (double)counts[1];
    if (kMode == 0) {
        head->sum_m = s_red[0];
        head->mean = s_red[0] / big_m;                                            // M = 0: NaN, and nothing is kept
    } else {
        head->sum_dev = s_red[0];
        head->std_dev = sqrt(s_red[0] / (big_m - 1.0));                           // M = 1: 0 / 0
        head->threshold = head->mean + std_ratio * head->std_dev;
        if (stats) { stats[0] = head->mean; stats[1] = head->std_dev; stats[2] = head->threshold; }
    }
}

__global__ void __launch_bounds__(kBlock)
occ_keep_kernel(Shape s, const uint64_t* __restrict__ cand, const double* __restrict__ m, const Head* __restrict__ head,
                uint64_t* __restrict__ surv, int64_t* __restrict__ counts) {
    const Where p = where(s);
    bool keep = false;
    if (bit_of(cand, p)) {
        const double x = m[p.v];
        keep = x > 0.0 && x < head->threshold;
    }
    const unsigned long long bits = __ballot(keep);
    if ((threadIdx.x & 63) == 0 && p.word < s.n_words) surv[p.word] = bits;
    wave_count(keep, counts + 2);
}

__global__ void __launch_bounds__(kBlock)
occ_core_kernel(Shape s, const uint64_t* __restrict__ surv, const float* __restrict__ ax, const float* __restrict__ ay,
                const float* __restrict__ az, int ball_r, double eps2, int min_points, uint64_t* __restrict__ core,
                int32_t* __restrict__ parent) {
    const Where p = where(s);
    bool is_core = false;
    if (bit_of(surv, p)) {
        const om::Grid g{surv, s.d, s.h, s.w, s.wpc};
        int count = 0;
        om::ball_visit(g, ax, ay, az, ball_r, eps2, p.i, p.j, p.k, [&](int, int, int) { return ++count < min_points; });
        is_core = count >= min_points;
    }
    if (p.inside) parent[p.v] = (int32_t)p.v;
    const unsigned long long bits = __ballot(is_core);
    if ((threadIdx.x & 63) == 0 && p.word < s.n_words) core[p.word] = bits;
}

__device__ __forceinline__ int32_t find_root(const int32_t* parent, int32_t v) {
    int32_t up = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
    while (up != v) {                                  // links go strictly downwards in index: at most v steps
        v = up;
        up = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
    }
    return v;
}
// find with pointer jumping for the union pass: every voxel on the way is pointed at its grandparent (atomicMin: a link only ever
// moves to a lower voxel of the same component, whoever else is writing it), which keeps the paths of a dense body short
__device__ __forceinline__ int32_t find_jump(int32_t* parent, int32_t v) {
    int32_t up = __atomic_load_n(parent + v, __ATOMIC_RELAXED);
    while (up != v) {                                  // strictly downwards in index: at most v steps
        const int32_t upup = __atomic_load_n(parent + up, __ATOMIC_RELAXED);
        if (upup != up) atomicMin(parent + v, upup);
        v = up;
        up = upup;
    }
    return v;
}
__device__ __forceinline__ void unite(int32_t* parent, int32_t a, int32_t b) {
    for (;;) {                                         // every retry strictly lowers a or b
        a = find_jump(parent, a);
        b = find_jump(parent, b);
        if (a == b) return;
        if (a < b) { const int32_t t = a; a = b; b = t; }
        const int32_t old = atomicMin(parent + a, b);  // a was a root (parent[a] == a) unless another lane linked it meanwhile:
        if (old == a) return;                          // then a hangs below min(old, b) and old and b are still to be joined
        a = old;
    }
}

__global__ void __launch_bounds__(kBlock)
occ_union_kernel(Shape s, const uint64_t* __restrict__ core, const float* __restrict__ ax, const float* __restrict__ ay,
                 const float* __restrict__ az, int ball_r, double eps2, int32_t* __restrict__ parent) {
    const Where p = where(s);
    if (!bit_of(core, p)) return;
    const om::Grid g{core, s.d, s.h, s.w, s.wpc};
    const int32_t v = (int32_t)p.v;
    om::ball_visit(g, ax, ay, az, ball_r, eps2, p.i, p.j, p.k, [&](int i2, int j2, int k2) {
        const int32_t u = (int32_t)(((int64_t)i2 * s.h + j2) * s.w + k2);
        if (u < v) unite(parent, v, u);
        return true;
    });
}

__global__ void __launch_bounds__(kBlock)
occ_flatten_kernel(Shape s, const uint64_t* __restrict__ core, int32_t* __restrict__ parent) {
    const Where p = where(s);
    if (!bit_of(core, p)) return;
    const int32_t r = find_root(parent, (int32_t)p.v);
    __atomic_store_n(parent + p.v, r, __ATOMIC_RELAXED);          // an ancestor replaces an ancestor: concurrent finds stay valid
}

__global__ void __launch_bounds__(kBlock)
occ_label_kernel(Shape s, const uint64_t* __restrict__ surv, const uint64_t* __restrict__ core, const float* __restrict__ ax,
                 const float* __restrict__ ay, const float* __restrict__ az, int ball_r, double eps2, const int32_t* __restrict__ parent,
                 int32_t* __restrict__ root, int32_t* __restrict__ sizes, int64_t* __restrict__ counts) {
    const Where p = where(s);
    int32_t r = -1;
    bool is_root = false;
    if (bit_of(core, p)) {
        r = parent[p.v];
        is_root = r == (int32_t)p.v;
    } else if (bit_of(surv, p)) {
        const om::Grid g{core, s.d, s.h, s.w, s.wpc};
        int32_t best = INT32_MAX;
        om::ball_visit(g, ax, ay, az, ball_r, eps2, p.i, p.j, p.k, [&](int i2, int j2, int k2) {
            const int32_t c = parent[((int64_t)i2 * s.h + j2) * s.w + k2];
            if (c < best) best = c;
            return true;
        });
        if (best != INT32_MAX) r = best;
    }
    if (p.inside) root[p.v] = r;
    // cluster sizes: the lanes of a wave mostly share a root, so one atomic per distinct root and wave (a body's voxels would
    // otherwise queue on one address)
    unsigned long long todo = __ballot(r >= 0);
    while (todo) {                                                                // wave-uniform; one distinct root per round
        const int leader = __ffsll((long long)todo) - 1;
        const int32_t lr = __shfl(r, leader, 64);
        const unsigned long long same = __ballot(r == lr) & todo;
        if ((int)(threadIdx.x & 63) == leader) atomicAdd(sizes + lr, __popcll(same));
        todo &= ~same;
    }
    wave_count(is_root, counts + 5);
}

__global__ void __launch_bounds__(kBlock)
occ_best_kernel(int64_t n, const int32_t* __restrict__ sizes, Head* __restrict__ head) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= n) return;
    const int32_t sz = sizes[v];
    if (sz > 0) atomicMax(&head->best, ((unsigned long long)(uint32_t)sz << 32) | (unsigned long long)(0xffffffffu - (uint32_t)v));
}

// keep: 0 = every voxel of a cluster, 1 = the largest cluster (everything if there is none), 2 = the bits themselves (no filters ran)
__global__ void __launch_bounds__(kBlock)
occ_mask_kernel(Shape s, const uint64_t* __restrict__ bits, const int32_t* __restrict__ root, const Head* __restrict__ head, int keep,
                uint8_t* __restrict__ mask, int64_t* __restrict__ counts) {
    const Where p = where(s);
    bool on = false;
    if (bit_of(bits, p)) {
        if (keep == 2) on = true;
        else if (keep == 0) on = root[p.v] >= 0;
        else {
            const unsigned long long best = head->best;
            on = best == 0ull ? true : root[p.v] == (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull));
        }
    }
    if (p.inside) mask[p.v] = on ? 1 : 0;
    wave_count(on, counts + 3);
    if (keep == 2) wave_count(on, counts + 2);
}

int shape_of(const pixie_occupancy_desc* desc, Shape& s, const char* who) {
    PX_REQUIRE(desc, "%s: null descriptor", who);
    PX_REQUIRE(desc->d >= 1 && desc->h >= 1 && desc->w >= 1, "%s: grid %d x %d x %d has a dimension < 1", who, desc->d, desc->h, desc->w);
    s.d = desc->d; s.h = desc->h; s.w = desc->w;
    s.wpc = om::words_per_column(s.w);
    s.n = (int64_t)s.d * s.h * s.w;
    s.n_words = (int64_t)s.d * s.h * s.wpc;
    PX_REQUIRE(s.n_words * 64 <= (int64_t)INT32_MAX - 64, "%s: grid %d x %d x %d exceeds the 2^31 voxels (last axis padded to 64) one call takes",
               who, s.d, s.h, s.w);
    return 0;
}

}  // namespace

extern "C" {

int64_t pixie_occupancy_scratch_bytes(const pixie_occupancy_desc* desc, int with_mean_dist) {
    Shape s;
    if (shape_of(desc, s, "pixie_occupancy_scratch_bytes")) return -1;
    return (int64_t)make_layout(s, !with_mean_dist).total_bytes;
}

int pixie_occupancy_mask(const pixie_occupancy_desc* desc, uint8_t* d_mask, double* d_mean_dist, int64_t* d_counts, void* d_scratch,
                         void* stream) {
    Shape s;
    if (shape_of(desc, s, "pixie_occupancy_mask")) return 1;
    PX_REQUIRE(desc->d_alphas && desc->d_rgb && desc->d_axis_x && desc->d_axis_y && desc->d_axis_z,
               "pixie_occupancy_mask: null pointer (d_alphas, d_rgb and the three axes are required)");
    PX_REQUIRE(d_mask && d_counts && d_scratch, "pixie_occupancy_mask: null pointer (d_mask, d_counts and d_scratch are required)");
    PX_REQUIRE(((uintptr_t)d_scratch & 15) == 0, "pixie_occupancy_mask: d_scratch must be 16-byte aligned");
    PX_REQUIRE(desc->dtype == 0 || desc->dtype == 1, "pixie_occupancy_mask: dtype %d is neither 0 (float16) nor 1 (float32)", desc->dtype);
    PX_REQUIRE(desc->keep == 0 || desc->keep == 1, "pixie_occupancy_mask: keep %d is neither 0 (non_noise) nor 1 (largest)", desc->keep);
    PX_REQUIRE(desc->nb_neighbors >= 1, "pixie_occupancy_mask: nb_neighbors %d < 1", desc->nb_neighbors);
    PX_REQUIRE(desc->min_points >= 1, "pixie_occupancy_mask: min_points %d < 1", desc->min_points);
    PX_REQUIRE(desc->eps_multiplier > 0.0 && std::isfinite(desc->eps_multiplier), "pixie_occupancy_mask: eps_multiplier %g is not a positive number",
               desc->eps_multiplier);
    PX_REQUIRE(desc->voxel_size > 0.0 && std::isfinite(desc->voxel_size), "pixie_occupancy_mask: voxel_size %g is not a positive number",
               desc->voxel_size);
    PX_REQUIRE(desc->lattice_spacing > 0.0 && std::isfinite(desc->lattice_spacing),
               "pixie_occupancy_mask: lattice_spacing %g is not a positive number", desc->lattice_spacing);
    PX_REQUIRE(std::isfinite(desc->std_ratio), "pixie_occupancy_mask: std_ratio is not finite");
    const double eps = desc->voxel_size * desc->eps_multiplier;
    const double reach_voxels = eps / desc->lattice_spacing;
    PX_REQUIRE(reach_voxels < (double)(om::kMaxBallR - 1), "pixie_occupancy_mask: eps of %g lattice spacings exceeds the %d one call takes",
               reach_voxels, om::kMaxBallR - 1);
    const int ball_r = om::ball_half_width(reach_voxels);
    const double eps2 = eps * eps;

    hipStream_t st = as_stream(stream);
    const Layout L = make_layout(s, d_mean_dist == nullptr);
    char* ws = (char*)d_scratch;
    Head* head = (Head*)ws;
    uint64_t* cand = (uint64_t*)(ws + L.cand);
    uint64_t* surv = (uint64_t*)(ws + L.surv);
    uint64_t* core = (uint64_t*)(ws + L.core);
    double* m = d_mean_dist ? d_mean_dist : (double*)(ws + L.m);
    int32_t* slow = (int32_t*)(ws + L.slow);
    int32_t* parent = (int32_t*)(ws + L.parent);
    int32_t* root = (int32_t*)(ws + L.root);
    int32_t* sizes = (int32_t*)(ws + L.sizes);
    double* partials = (double*)(ws + L.partials);
    const float *ax = desc->d_axis_x, *ay = desc->d_axis_y, *az = desc->d_axis_z;
    const dim3 grid((unsigned)cdiv(s.n_words * 64, kBlock)), block(kBlock);

    PX_CHECK_HIP(hipMemsetAsync(d_counts, 0, 8 * sizeof(int64_t), st));
    PX_CHECK_HIP(hipMemsetAsync(head, 0, kHeadBytes, st));
    if (desc->dtype == 0)
        hipLaunchKernelGGL(occ_classify_kernel<__half>, grid, block, 0, st, s, (const __half*)desc->d_alphas, (const __half*)desc->d_rgb,
                           (float)desc->alpha_threshold, (float)desc->gray_threshold, cand, d_counts);
    else
        hipLaunchKernelGGL(occ_classify_kernel<float>, grid, block, 0, st, s, (const float*)desc->d_alphas, (const float*)desc->d_rgb,
                           (float)desc->alpha_threshold, (float)desc->gray_threshold, cand, d_counts);
    PX_CHECK_HIP(hipGetLastError());
    if (!desc->run_filters) {                          // voxelize.py:252-253: the thresholds alone; d_mean_dist and d_stats stay untouched
        hipLaunchKernelGGL(occ_mask_kernel, grid, block, 0, st, s, cand, root, head, 2, d_mask, d_counts);
        PX_CHECK_HIP(hipGetLastError());
        return 0;
    }
    hipLaunchKernelGGL(occ_fast_kernel, grid, block, 0, st, s, cand, ax, ay, az, desc->nb_neighbors, d_counts, m, slow, head);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(occ_slow_kernel, dim3(kSlowBlocks), block, 0, st, s, cand, ax, ay, az, desc->nb_neighbors, d_counts, m, slow, head);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(occ_reduce_kernel<0>, dim3(kReduceBlocks), block, 0, st, s.n, m, head, partials);
    hipLaunchKernelGGL(occ_finish_kernel<0>, dim3(1), dim3(kReduceBlocks), 0, st, partials, d_counts, desc->std_ratio, head, desc->d_stats);
    hipLaunchKernelGGL(occ_reduce_kernel<1>, dim3(kReduceBlocks), block, 0, st, s.n, m, head, partials);
    hipLaunchKernelGGL(occ_finish_kernel<1>, dim3(1), dim3(kReduceBlocks), 0, st, partials, d_counts, desc->std_ratio, head, desc->d_stats);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(occ_keep_kernel, grid, block, 0, st, s, cand, m, head, surv, d_counts);
    PX_CHECK_HIP(hipGetLastError());
    PX_CHECK_HIP(hipMemsetAsync(sizes, 0, 4 * (size_t)s.n, st));
    hipLaunchKernelGGL(occ_core_kernel, grid, block, 0, st, s, surv, ax, ay, az, ball_r, eps2, desc->min_points, core, parent);
    hipLaunchKernelGGL(occ_union_kernel, grid, block, 0, st, s, core, ax, ay, az, ball_r, eps2, parent);
    hipLaunchKernelGGL(occ_flatten_kernel, grid, block, 0, st, s, core, parent);
    hipLaunchKernelGGL(occ_label_kernel, grid, block, 0, st, s, surv, core, ax, ay, az, ball_r, eps2, parent, root, sizes, d_counts);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(occ_best_kernel, dim3((unsigned)cdiv(s.n, kBlock)), block, 0, st, s.n, sizes, head);
    hipLaunchKernelGGL(occ_mask_kernel, grid, block, 0, st, s, surv, root, head, desc->keep, d_mask, d_counts);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // extern "C"
