// tests/host_harness/knn_math_host.cpp -- compiles pixie_amd/csrc/knn_math.h for the HOST so that CPU-only tests can check the
// arithmetic of distCUDA2 before any GPU run: the same header functions in the same order as the kernels of knn.hip (bounding box,
// Morton codes, a stable sort, a box per group of consecutive sorted points, own group first, then every group whose box can still
// hold a closer point for some member), as one sequential loop.  `group` is a parameter here so that small clouds span many boxes.
// Test infrastructure only: the product never executes this.
#include <stdint.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "../../pixie_amd/csrc/knn_math.h"

namespace km = pixie::knn;

extern "C" {

void hh_knn_morton(int n, const float* p, const float* lo, const float* hi, uint32_t* codes) {
    for (int i = 0; i < n; ++i) codes[i] = km::morton3(p + 3 * i, lo, hi);
}

// out[n]; visited (if given) receives the number of distances evaluated, so that a test can see that pruning took place
int hh_knn_mean_dist2(int n, const float* p, int group, float* out, int64_t* visited) {
    if (n == 0) return 0;
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < n; ++i)
        for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], p[3 * i + d]); hi[d] = fmaxf(hi[d], p[3 * i + d]); }
    std::vector<uint32_t> codes(n);
    hh_knn_morton(n, p, lo, hi, codes.data());
    std::vector<int> order(n);
    std::iota(order.begin(), order.end(), 0);
    std::stable_sort(order.begin(), order.end(), [&](int a, int b) { return codes[a] < codes[b]; });
    const int groups = (n + group - 1) / group;
    std::vector<float> blo(3 * groups, INFINITY), bhi(3 * groups, -INFINITY);
    for (int s = 0; s < n; ++s)
        for (int d = 0; d < 3; ++d) {
            const float v = p[3 * order[s] + d];
            blo[3 * (s / group) + d] = fminf(blo[3 * (s / group) + d], v);
            bhi[3 * (s / group) + d] = fmaxf(bhi[3 * (s / group) + d], v);
        }
    int64_t count = 0;
    std::vector<float> best(3 * group);
    for (int g = 0; g < groups; ++g) {
        const int s0 = g * group, s1 = std::min(n, s0 + group);
        std::fill(best.begin(), best.end(), FLT_MAX);
        for (int s = s0; s < s1; ++s) {
            const float* me = p + 3 * order[s];
            float* b = &best[3 * (s - s0)];
            for (int t = s0; t < s1; ++t) {
                if (t == s) continue;
                const float* q = p + 3 * order[t];
                km::insert3(km::dist2(me[0], me[1], me[2], q[0], q[1], q[2]), b[0], b[1], b[2]);
                ++count;
            }
        }
        for (int o = 0; o < groups; ++o) {
            if (o == g) continue;
            float reach = 0.0f;
            for (int s = s0; s < s1; ++s) reach = fmaxf(reach, best[3 * (s - s0) + 2]);
            if (!(km::box_box_dist2(&blo[3 * g], &bhi[3 * g], &blo[3 * o], &bhi[3 * o]) <= reach)) continue;
            const int t0 = o * group, t1 = std::min(n, t0 + group);
            for (int s = s0; s < s1; ++s) {
                const float* me = p + 3 * order[s];
                float* b = &best[3 * (s - s0)];
                // the per-point bound must never exceed a member's distance; it is used here to prune further, as a check of it
                if (km::box_point_dist2(&blo[3 * o], &bhi[3 * o], me[0], me[1], me[2]) > b[2]) continue;
                for (int t = t0; t < t1; ++t) {
                    const float* q = p + 3 * order[t];
                    km::insert3(km::dist2(me[0], me[1], me[2], q[0], q[1], q[2]), b[0], b[1], b[2]);
                    ++count;
                }
            }
        }
        for (int s = s0; s < s1; ++s) out[order[s]] = km::mean3(best[3 * (s - s0)], best[3 * (s - s0) + 1], best[3 * (s - s0) + 2]);
    }
    if (visited) *visited = count;
    return 0;
}

}  // extern "C"
