// pixie_amd/csrc/occupancy_math.h -- arithmetic of the occupancy mask (pixie/voxel/voxelize.py:_create_occupancy_mask): density and
// gray thresholds, Open3D's statistical outlier removal and its DBSCAN, restated on the voxel lattice.
//
// __host__ __device__ like knn_math.h: the kernels of occupancy.hip run it and tests/host_harness/occupancy_math_host.cpp runs the
// same functions on the CPU.  Both sides are built with -ffp-contract=off.
//
// The candidates live in a bit grid: voxel (i, j, k) of a (D, H, W) grid is bit k & 63 of word (i H + j) wpc + (k >> 6), wpc =
// ceil(W / 64); bits at k >= W are zero.  Voxel (i, j, k) sits at (axis_x[i], axis_y[j], axis_z[k]), float32 coordinates whose
// spacing is the same on the three axes up to rounding.  Distances are float64 on those float32 values:
//   dist2_axes()     ((dx dx + dy dy) + dz dz), d = difference of the float32 coordinates, in float64
//
// Stage A
//   classify()       float32(alpha) > float32(alpha_threshold) and ((r + g) + b) / 3 > float32(gray_threshold), float32 throughout
//
// Stage B: the mean distance of a voxel to its k' nearest candidates, itself included.  On a lattice the nearest candidates are
// whole shells of integer squared offset n = di^2 + dj^2 + dk^2: two offsets of different n differ in length by at least
// spacing / (2 sqrt(n) + 1), far more than the rounding of the axes, so ascending n IS ascending distance and only the choice inside
// the last shell is free (Open3D's k-d tree breaks those ties by its own traversal order).
//   kOffsets         the offsets with n <= kFastR2, sorted by n, then (di, dj, dk)
//   fast_mean()      walks kOffsets shell by shell; done as soon as a complete shell brings the count to k'.  Neighbours of the last
//                    shell are taken in table order.  Fails (returns false) when the table runs out first.
//   The slow path, for the voxels fast_mean() gives up on, scans a clipped cube of half-width r word by word:
//   word_count_le()  candidates of one 64-bit word with n <= T, by mask arithmetic (no loop over bits)
//   word_sum_lt()    sum of the true distances of one word's candidates with n < T, and the word's candidates with n == T
//   A ball of squared radius T <= r^2 lies inside the cube, so the smallest T whose count reaches k' is found by bisection, the
//   distances with n < T are summed and the first k' - count(n < T) candidates with n == T in scan order complete the set.
//
// Stage C: DBSCAN with Open3D's open ball.
//   ball_visit()     calls f(i2, j2, k2) for every set bit of a grid with ((dx dx + dy dy) + dz dz) < eps^2, decided by that float64
//                    comparison on the coordinates and not by integer offsets; the bit grid only says where to look.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define OCC_HD __host__ __device__ __forceinline__
#else
#define OCC_HD inline
#endif

namespace pixie {
namespace occ {

constexpr int kFastR = 3;                 // half-width of the fast path's neighbourhood
constexpr int kFastR2 = 9;                // largest integer squared offset in kOffsets
constexpr int kMaxOffsets = 128;
constexpr int kMaxBallR = 31;             // 2 R + 1 bits of one row must fit a 64-bit window

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
static_assert(kOffsets.count == 123, "offsets with di^2 + dj^2 + dk^2 <= 9");

struct Grid {
    const uint64_t* words;
    int d, h, w, wpc;
};

OCC_HD int words_per_column(int w) { return (w + 63) >> 6; }

OCC_HD bool classify(float alpha, float r, float g, float b, float alpha_threshold, float gray_threshold, bool* dense) {
    *dense = alpha > alpha_threshold;
    const float mean = ((r + g) + b) / 3.0f;
    return *dense && mean > gray_threshold;
}

OCC_HD bool test_bit(const Grid& g, int i, int j, int k) {
    if ((unsigned)i >= (unsigned)g.d || (unsigned)j >= (unsigned)g.h || (unsigned)k >= (unsigned)g.w) return false;
    return (g.words[((size_t)i * g.h + j) * g.wpc + (k >> 6)] >> (k & 63)) & 1u;
}

// 64 bits of row (i, j) starting at k0, which may lie outside [0, W): bit b is voxel k0 + b, zero outside the grid
OCC_HD uint64_t window(const Grid& g, int i, int j, int k0) {
    const uint64_t* row = g.words + ((size_t)i * g.h + j) * g.wpc;
    const int w0 = k0 >> 6, sh = k0 & 63;                         // arithmetic shift: floor for negative k0
    const uint64_t a = (w0 >= 0 && w0 < g.wpc) ? row[w0] : 0ull;
    if (sh == 0) return a;
    const uint64_t b = (w0 + 1 >= 0 && w0 + 1 < g.wpc) ? row[w0 + 1] : 0ull;
    return (a >> sh) | (b << (64 - sh));
}

OCC_HD double dist2_axes(const float* ax, const float* ay, const float* az, int i, int j, int k, int i2, int j2, int k2) {
    const double dx = (double)ax[i2] - (double)ax[i], dy = (double)ay[j2] - (double)ay[j], dz = (double)az[k2] - (double)az[k];
    return (dx * dx + dy * dy) + dz * dz;
}

// mean distance to the kprime (>= 1) nearest candidates out of kOffsets; false: the table ran out, *mean is untouched
OCC_HD bool fast_mean(const Grid& g, const OffsetTable* tab, const float* ax, const float* ay, const float* az, int i, int j, int k,
                      int kprime, double* mean) {
    int count = 0, t = 0;
    double sum = 0.0;
    while (t < tab->count) {
        const int n = tab->at[t].n;
        for (; t < tab->count && tab->at[t].n == n; ++t) {
            const int i2 = i + tab->at[t].di, j2 = j + tab->at[t].dj, k2 = k + tab->at[t].dk;
            if (!test_bit(g, i2, j2, k2)) continue;
            if (count < kprime) sum += sqrt(dist2_axes(ax, ay, az, i, j, k, i2, j2, k2));
            ++count;
        }
        if (count >= kprime) {
            *mean = sum / (double)kprime;
            return true;
        }
    }
    return false;
}

OCC_HD int64_t isqrt64(int64_t v) {
    int64_t r = (int64_t)sqrt((double)v);
    while (r * r > v) --r;
    while ((r + 1) * (r + 1) <= v) ++r;
    return r;
}

// bits of `word` (bit b = voxel k0 + b of a row at integer squared offset `base` in the other two axes) with base + (k - ck)^2 <= T
OCC_HD uint64_t word_mask_le(int k0, int ck, int64_t base, int64_t T) {
    if (base > T) return 0ull;
    const int64_t rr = isqrt64(T - base);
    int64_t lo = (int64_t)ck - rr - k0, hi = (int64_t)ck + rr - k0;       // bit positions, inclusive
    if (hi < 0 || lo > 63) return 0ull;
    if (lo < 0) lo = 0;
    if (hi > 63) hi = 63;
    const uint64_t upto_hi = hi == 63 ? ~0ull : ((1ull << (hi + 1)) - 1ull);
    return upto_hi & ~((1ull << lo) - 1ull);
}
OCC_HD int word_count_le(uint64_t word, int k0, int ck, int64_t base, int64_t T) {
    return __builtin_popcountll(word & word_mask_le(k0, ck, base, T));
}

// One word of row (i2, j2) seen from voxel (i, j, k): adds the distances of its candidates with n < T to *sum, returns their number,
// and leaves the candidates with n == T (at most two) in *ties.
OCC_HD int word_sum_lt(uint64_t word, int k0, const float* ax, const float* ay, const float* az, int i, int j, int k, int i2, int j2,
                       int64_t base, int64_t T, double* sum, uint64_t* ties) {
    uint64_t m = word & word_mask_le(k0, k, base, T);
    int count = 0;
    *ties = 0ull;
    while (m) {
        const int b = __builtin_ctzll(m);
        m &= m - 1;
        const int k2 = k0 + b;
        const int64_t dk = k2 - k;
        if (base + dk * dk == T) { *ties |= 1ull << b; continue; }
        *sum += sqrt(dist2_axes(ax, ay, az, i, j, k, i2, j2, k2));
        ++count;
    }
    return count;
}

// f(i2, j2, k2) -> bool (false stops the visit) for every set bit of g inside the open ball of squared radius eps2 around (i, j, k),
// the centre included if its bit is set.  R >= any index offset that can lie inside the ball, R <= kMaxBallR.
template <class F>
OCC_HD void ball_visit(const Grid& g, const float* ax, const float* ay, const float* az, int R, double eps2, int i, int j, int k, F&& f) {
    const uint64_t span = (2 * R + 1 == 64) ? ~0ull : ((1ull << (2 * R + 1)) - 1ull);
    const double x = (double)ax[i], y = (double)ay[j], z = (double)az[k];
    for (int i2 = (i - R < 0 ? 0 : i - R); i2 <= i + R && i2 < g.d; ++i2) {
        const double dx = (double)ax[i2] - x;
        for (int j2 = (j - R < 0 ? 0 : j - R); j2 <= j + R && j2 < g.h; ++j2) {
            const double dy = (double)ay[j2] - y;
            const double a = dx * dx + dy * dy;
            if (!(a < eps2)) continue;                             // a + dz dz >= a: rounding is monotone
            uint64_t m = window(g, i2, j2, k - R) & span;
            while (m) {
                const int b = __builtin_ctzll(m);
                m &= m - 1;
                const int k2 = k - R + b;
                const double dz = (double)az[k2] - z;
                if ((a + dz * dz) < eps2)
                    if (!f(i2, j2, k2)) return;
            }
        }
    }
}

// half-width of the index cube that holds every voxel of an open ball of eps_multiplier voxel sizes: one more than its integer part,
// which leaves a whole voxel of margin for the rounding of the axes
OCC_HD int ball_half_width(double eps_multiplier) { return (int)floor(eps_multiplier) + 1; }

}  // namespace occ
}  // namespace pixie
