// tests/host_harness/part_seg_math_host.cpp -- compiles pixie_amd/csrc/part_seg_math.h for the HOST so that CPU-only tests can check
// the arithmetic of the part segmentation before any GPU run: the same header functions in the same order as the kernels of
// part_segmentation.hip (the query norm by 256 partial sums and their tree; per masked voxel the 64 lanes' shares of the square sum
// and of the K dot products, the xor butterfly, the epilogue; fast_vote over the sorted offset table and, for the voxels it gives up
// on, the doubling cube, the bisection of the integer squared radius and the last shell in C order; the material rows), as
// sequential loops.  Test infrastructure only: the product never executes this.
#include <stdint.h>

#include <algorithm>
#include <cmath>
#include <vector>

#include "../../pixie_amd/csrc/part_seg_math.h"

namespace pm = pixie::pseg;

namespace {

int64_t cube_count_le(const pm::LabelGrid& g, const pm::Cube& c, int ci, int cj, int ck, int64_t T) {
    int64_t cnt = 0;
    for (int64_t q = 0; q < c.items; ++q) {
        int64_t n;
        const int l = pm::cube_item(g, c, q, ci, cj, ck, &n);
        cnt += (l >= 0 && n <= T) ? 1 : 0;
    }
    return cnt;
}

int slow_vote(const pm::LabelGrid& g, int ci, int cj, int ck, int kprime) {
    const int reach = std::max(g.d, std::max(g.h, g.w));
    int64_t r = pm::kFastR + 1, lo = pm::kFastR2 + 1, hi;                      // the table held too few: T > kFastR2
    for (;;) {
        if (r >= reach) {
            const int64_t a = std::max(ci, g.d - 1 - ci), b = std::max(cj, g.h - 1 - cj), cc = std::max(ck, g.w - 1 - ck);
            hi = a * a + b * b + cc * cc;
            break;
        }
        hi = r * r;
        if (cube_count_le(g, pm::cube_of(g, ci, cj, ck, r), ci, cj, ck, hi) >= kprime) break;
        lo = hi + 1;
        r *= 2;
    }
    while (lo < hi) {
        const int64_t mid = lo + (hi - lo) / 2;
        if (cube_count_le(g, pm::cube_for(g, ci, cj, ck, mid), ci, cj, ck, mid) >= kprime) hi = mid; else lo = mid + 1;
    }
    const int64_t T = lo;
    const int64_t below = T > 0 ? cube_count_le(g, pm::cube_for(g, ci, cj, ck, T - 1), ci, cj, ck, T - 1) : 0;
    int64_t need = kprime - below;
    pm::Tally tally;
    pm::tally_clear(tally);
    const pm::Cube c = pm::cube_for(g, ci, cj, ck, T);
    for (int64_t q = 0; q < c.items; ++q) {                                    // C order
        int64_t n;
        const int l = pm::cube_item(g, c, q, ci, cj, ck, &n);
        if (l < 0) continue;
        if (n < T) pm::tally_add(tally, l);
        else if (n == T && need > 0) { pm::tally_add(tally, l); --need; }
    }
    return pm::tally_mode(tally);
}

}  // namespace

extern "C" {

int hh_ps_offsets(int8_t* out) {                                               // [kMaxOffsets][4]: di, dj, dk, n
    for (int t = 0; t < pm::kOffsets.count; ++t) {
        out[4 * t] = pm::kOffsets.at[t].di; out[4 * t + 1] = pm::kOffsets.at[t].dj; out[4 * t + 2] = pm::kOffsets.at[t].dk;
        out[4 * t + 3] = pm::kOffsets.at[t].n;
    }
    return pm::kOffsets.count;
}

float hh_ps_half(uint16_t h) { return pm::half_to_float(h); }

// stage A over a (d, h, w, channels) float16 grid; labels / scores as the kernels leave them, counts[kMaxParts + 1]
int hh_ps_stage_a(int d, int h, int w, int channels, int parts, const uint16_t* features, const uint8_t* mask, const float* queries,
                  float temperature, int8_t* labels, float* scores, int64_t* counts) {
    if (channels % 8 || channels > pm::kMaxChannels || parts < 1 || parts > pm::kMaxParts) return 1;
    const int64_t n = (int64_t)d * h * w;
    const int n_chunks = channels / 8;
    std::vector<float> qn((size_t)parts * channels);
    for (int j = 0; j < parts; ++j) {
        double part[pm::kNormThreads];
        for (int t = 0; t < pm::kNormThreads; ++t) part[t] = pm::query_sq_part(queries + (size_t)j * channels, channels, t);
        pm::tree_sum(part, pm::kNormThreads);
        const float norm = pm::norm_of(part[0]);
        for (int e = 0; e < channels; ++e) qn[(size_t)j * channels + e] = queries[(size_t)j * channels + e] / norm;
    }
    for (int j = 0; j <= pm::kMaxParts; ++j) counts[j] = 0;
    std::vector<float> f((size_t)64 * 8 * pm::kMaxChunks);
    for (int64_t v = 0; v < n; ++v) {
        if (!mask[v]) { labels[v] = -1; scores[v] = NAN; continue; }
        const uint16_t* row = features + (size_t)v * channels;
        for (int lane = 0; lane < 64; ++lane)
            for (int m = 0; m < pm::kMaxChunks; ++m) {
                const int chunk = lane + 64 * m;
                for (int e = 0; e < 8; ++e)
                    f[((size_t)lane * pm::kMaxChunks + m) * 8 + e] = chunk < n_chunks ? pm::half_to_float(row[8 * chunk + e]) : 0.0f;
            }
        float lanes[64], dots[pm::kMaxParts];
        for (int lane = 0; lane < 64; ++lane) lanes[lane] = pm::lane_dot(&f[(size_t)lane * 8 * pm::kMaxChunks], nullptr, lane, n_chunks);
        pm::butterfly(lanes);
        const float sq = lanes[0];
        for (int j = 0; j < parts; ++j) {
            for (int lane = 0; lane < 64; ++lane)
                lanes[lane] = pm::lane_dot(&f[(size_t)lane * 8 * pm::kMaxChunks], &qn[(size_t)j * channels], lane, n_chunks);
            pm::butterfly(lanes);
            dots[j] = lanes[0];
        }
        float score;
        const int label = pm::epilogue(dots, parts, sq, temperature, &score);
        labels[v] = (int8_t)label;
        scores[v] = score;
        ++counts[label];
        ++counts[pm::kMaxParts];
    }
    return 0;
}

// stage B over the labels of stage A; returns the number of voxels that left the fast path
int64_t hh_ps_vote(int d, int h, int w, const int8_t* labels, int vote_k, int8_t* voted) {
    const pm::LabelGrid g{labels, d, h, w};
    const int64_t n = (int64_t)d * h * w;
    int64_t masked = 0, slow = 0;
    for (int64_t v = 0; v < n; ++v) masked += labels[v] >= 0;
    const int kprime = (int)std::min<int64_t>(vote_k, masked);
    for (int64_t v = 0; v < n; ++v) {
        if (labels[v] < 0) { voted[v] = -1; continue; }
        const int ck = (int)(v % w), cj = (int)((v / w) % h), ci = (int)(v / ((int64_t)w * h));
        int label = 0;
        if (!pm::fast_vote(g, &pm::kOffsets, ci, cj, ck, kprime, &label)) {
            label = slow_vote(g, ci, cj, ck, kprime);
            ++slow;
        }
        voted[v] = (int8_t)label;
    }
    return slow;
}

void hh_ps_material(int64_t n, const int8_t* labels, const float* props, int parts, float background_id, float* material) {
    for (int64_t v = 0; v < n; ++v) pm::material_row(props, labels[v] < parts ? labels[v] : -1, background_id, material + 4 * v);
}

}  // extern "C"
