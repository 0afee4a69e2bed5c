// tests/host_harness/occupancy_math_host.cpp -- compiles pixie_amd/csrc/occupancy_math.h for the HOST so that CPU-only tests can
// check the arithmetic of the occupancy mask before any GPU run: the same header functions in the same order as the kernels of
// occupancy.hip (classify into a bit grid; fast_mean over the sorted offset table; for the voxels it gives up on, the doubling cube,
// the bisection of the integer squared radius with word_count_le and the tie-completed sum with word_sum_lt; two reductions; the
// open-ball core test, union-find with links towards the lower index, border labels and both keep rules through ball_visit), as
// sequential loops.  Test infrastructure only: the product never executes this.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../pixie_amd/csrc/occupancy_math.h"

namespace om = pixie::occ;

namespace {

int find_root(std::vector<int32_t>& parent, int v) {
    while (parent[v] != v) v = parent[v];
    return v;
}

int64_t cube_count_le(const om::Grid& g, int i0, int i1, int j0, int j1, int w0, int w1, int ci, int cj, int ck, int64_t T) {
    int64_t cnt = 0;
    for (int i2 = i0; i2 <= i1; ++i2)
        for (int j2 = j0; j2 <= j1; ++j2)
            for (int wi = w0; wi <= w1; ++wi) {
                const int64_t di = i2 - ci, dj = j2 - cj;
                cnt += om::word_count_le(g.words[((size_t)i2 * g.h + j2) * g.wpc + wi], wi * 64, ck, di * di + dj * dj, T);
            }
    return cnt;
}

struct Cube { int i0, i1, j0, j1, w0, w1; };
Cube cube_of(const om::Grid& g, int ci, int cj, int ck, int64_t r) {
    const int rr = (int)std::min<int64_t>(r, INT32_MAX / 2);
    return {std::max(ci - rr, 0), std::min(ci + rr, g.d - 1), std::max(cj - rr, 0), std::min(cj + rr, g.h - 1), std::max(ck - rr, 0) >> 6,
            std::min(ck + rr, g.w - 1) >> 6};
}
int64_t count_le(const om::Grid& g, const Cube& c, int ci, int cj, int ck, int64_t T) {
    return cube_count_le(g, c.i0, c.i1, c.j0, c.j1, c.w0, c.w1, ci, cj, ck, T);
}

double slow_mean(const om::Grid& g, const float* ax, const float* ay, const float* az, int ci, int cj, int ck, int kprime) {
    const int reach = std::max(g.d, std::max(g.h, g.w));
    int r = om::kFastR + 1;
    int64_t lo = 0, hi;
    for (;;) {
        if (r >= reach) {
            const int64_t a = std::max(ci, g.d - 1 - ci), b = std::max(cj, g.h - 1 - cj), c = std::max(ck, g.w - 1 - ck);
            hi = a * a + b * b + c * c;
            break;
        }
        hi = (int64_t)r * r;
        if (count_le(g, cube_of(g, ci, cj, ck, r), ci, cj, ck, hi) >= kprime) break;
        lo = hi + 1;
        r *= 2;
    }
    while (lo < hi) {                                              // every probe scans the cube of half-width floor(sqrt(T)), as the kernel
        const int64_t mid = lo + (hi - lo) / 2;
        if (count_le(g, cube_of(g, ci, cj, ck, om::isqrt64(mid)), ci, cj, ck, mid) >= kprime) hi = mid; else lo = mid + 1;
    }
    const int64_t T = lo;
    int64_t need = kprime - (T > 0 ? count_le(g, cube_of(g, ci, cj, ck, om::isqrt64(T - 1)), ci, cj, ck, T - 1) : 0);
    const Cube c = cube_of(g, ci, cj, ck, om::isqrt64(T));
    double sum = 0.0;
    for (int i2 = c.i0; i2 <= c.i1; ++i2)                          // the kernel's scan order: rows, then words, then bits
        for (int j2 = c.j0; j2 <= c.j1; ++j2)
            for (int wi = c.w0; wi <= c.w1; ++wi) {
                const int64_t di = i2 - ci, dj = j2 - cj;
                uint64_t ties = 0;
                om::word_sum_lt(g.words[((size_t)i2 * g.h + j2) * g.wpc + wi], wi * 64, ax, ay, az, ci, cj, ck, i2, j2, di * di + dj * dj, T,
                                &sum, &ties);
                while (ties) {
                    const int b = __builtin_ctzll(ties);
                    ties &= ties - 1;
                    if (need > 0) { sum += sqrt(om::dist2_axes(ax, ay, az, ci, cj, ck, i2, j2, wi * 64 + b)); --need; }
                }
            }
    return sum / (double)kprime;
}

}  // namespace

extern "C" {

int hh_occ_offsets(int8_t* out /* [count][4] */) {
    for (int t = 0; t < om::kOffsets.count; ++t) {
        out[4 * t] = om::kOffsets.at[t].di; out[4 * t + 1] = om::kOffsets.at[t].dj; out[4 * t + 2] = om::kOffsets.at[t].dk;
        out[4 * t + 3] = om::kOffsets.at[t].n;
    }
    return om::kOffsets.count;
}

// alphas [d h w], rgb [d h w 3] float32 (the float16 files widen exactly).  Outputs per voxel: cand, stage_b, non_noise, largest
// (0 / 1), m (NaN off the candidates), root (-1: noise or no survivor); counts[8] and stats[3] as pixie_occupancy_mask fills them.
int hh_occ_mask(int d, int h, int w, const float* alphas, const float* rgb, const float* ax, const float* ay, const float* az,
                double voxel_size, double lattice_spacing, double alpha_threshold, double gray_threshold, int nb_neighbors, double std_ratio,
                int min_points, double eps_multiplier, uint8_t* cand_out, double* m, uint8_t* stage_b, int32_t* root, uint8_t* non_noise,
                uint8_t* largest, int64_t* counts, double* stats) {
    const int wpc = om::words_per_column(w);
    const int64_t n = (int64_t)d * h * w;
    std::vector<uint64_t> cand((size_t)d * h * wpc, 0), surv(cand.size(), 0), core(cand.size(), 0);
    for (int t = 0; t < 8; ++t) counts[t] = 0;
    auto index = [&](int i, int j, int k) { return ((int64_t)i * h + j) * w + k; };
    auto set_bit = [&](std::vector<uint64_t>& b, int i, int j, int k) { b[((size_t)i * h + j) * wpc + (k >> 6)] |= 1ull << (k & 63); };
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                const int64_t v = index(i, j, k);
                bool dense = false;
                const bool keep = om::classify(alphas[v], rgb[3 * v], rgb[3 * v + 1], rgb[3 * v + 2], (float)alpha_threshold,
                                               (float)gray_threshold, &dense);
                counts[0] += dense; counts[1] += keep;
                cand_out[v] = keep;
                if (keep) set_bit(cand, i, j, k);
            }
    const om::Grid gc{cand.data(), d, h, w, wpc};
    const int kprime = (int)std::min<int64_t>(nb_neighbors, counts[1]);
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                const int64_t v = index(i, j, k);
                m[v] = NAN;
                if (!om::test_bit(gc, i, j, k)) continue;
                double mean = 0.0;
                if (!om::fast_mean(gc, &om::kOffsets, ax, ay, az, i, j, k, kprime, &mean)) {
                    mean = slow_mean(gc, ax, ay, az, i, j, k, kprime);
                    ++counts[4];
                }
                m[v] = mean;
            }
    double sum = 0.0;
    for (int64_t v = 0; v < n; ++v) if (m[v] == m[v]) sum += m[v];
    const double cloud_mean = sum / (double)counts[1];
    double dev = 0.0;
    for (int64_t v = 0; v < n; ++v) if (m[v] == m[v]) dev += (m[v] - cloud_mean) * (m[v] - cloud_mean);
    const double std_dev = sqrt(dev / ((double)counts[1] - 1.0));
    const double threshold = cloud_mean + std_ratio * std_dev;
    stats[0] = cloud_mean; stats[1] = std_dev; stats[2] = threshold;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                const int64_t v = index(i, j, k);
                const bool keep = om::test_bit(gc, i, j, k) && m[v] > 0.0 && m[v] < threshold;
                stage_b[v] = keep;
                counts[2] += keep;
                if (keep) set_bit(surv, i, j, k);
            }
    const om::Grid gs{surv.data(), d, h, w, wpc};
    const double eps = voxel_size * eps_multiplier, eps2 = eps * eps;
    const int R = om::ball_half_width(eps / lattice_spacing);
    if (R > om::kMaxBallR) return 1;
    std::vector<int32_t> parent((size_t)n), sizes((size_t)n, 0);
    for (int64_t v = 0; v < n; ++v) parent[v] = (int32_t)v;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                if (!om::test_bit(gs, i, j, k)) continue;
                int count = 0;
                om::ball_visit(gs, ax, ay, az, R, eps2, i, j, k, [&](int, int, int) { return ++count < min_points; });
                if (count >= min_points) set_bit(core, i, j, k);
            }
    const om::Grid gk{core.data(), d, h, w, wpc};
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                if (!om::test_bit(gk, i, j, k)) continue;
                const int32_t v = (int32_t)index(i, j, k);
                om::ball_visit(gk, ax, ay, az, R, eps2, i, j, k, [&](int i2, int j2, int k2) {
                    const int32_t u = (int32_t)index(i2, j2, k2);
                    if (u < v) {
                        int a = find_root(parent, v), b = find_root(parent, u);
                        if (a != b) parent[std::max(a, b)] = std::min(a, b);
                    }
                    return true;
                });
            }
    unsigned long long best = 0;
    for (int i = 0; i < d; ++i)
        for (int j = 0; j < h; ++j)
            for (int k = 0; k < w; ++k) {
                const int64_t v = index(i, j, k);
                int32_t r = -1;
                if (om::test_bit(gk, i, j, k)) {
                    r = find_root(parent, (int)v);
                    counts[5] += r == (int32_t)v;
                } else if (om::test_bit(gs, i, j, k)) {
                    int32_t low = INT32_MAX;
                    om::ball_visit(gk, ax, ay, az, R, eps2, i, j, k, [&](int i2, int j2, int k2) {
                        low = std::min(low, (int32_t)find_root(parent, (int)index(i2, j2, k2)));
                        return true;
                    });
                    if (low != INT32_MAX) r = low;
                }
                root[v] = r;
                if (r >= 0) ++sizes[r];
            }
    for (int64_t v = 0; v < n; ++v)
        if (sizes[v] > 0) best = std::max(best, ((unsigned long long)(uint32_t)sizes[v] << 32) | (0xffffffffu - (uint32_t)v));
    for (int64_t v = 0; v < n; ++v) {
        non_noise[v] = stage_b[v] && root[v] >= 0;
        largest[v] = stage_b[v] && (best == 0 ? true : root[v] == (int32_t)(0xffffffffu - (uint32_t)(best & 0xffffffffull)));
        counts[3] += non_noise[v];
    }
    return 0;
}

}  // extern "C"
