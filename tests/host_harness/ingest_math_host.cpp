// tests/host_harness/ingest_math_host.cpp -- compiles pixie_amd/csrc/ingest_math.h for the HOST so that CPU-only tests can check
// the scene ingest's arithmetic before any GPU run: the same header functions in the same order as the kernels of
// scene_ingest.hip (classify + bound, then a stable compaction), as one sequential loop.
// Test infrastructure only: the product never executes this.
#include <stdint.h>

#include "../../pixie_amd/csrc/ingest_math.h"

namespace im = pixie::ingest;

extern "C" {
// cols: 11 + 3 K entries as pixie_scene_ingest takes them.  Outputs have n rows of room; counts = selected, unselected, dropped.
// Returns 0, or 2 (nothing selected) / 3 (zero extent) as the library does.
int hh_ingest(int64_t n, int n_attr, const float* block, const int32_t* cols, int K, int n_rot, const float* rot, int has_area,
              const float* area, float opacity_threshold, float z_shift, int32_t* cls_out, float* pos, float* cov, float* opacity,
              float* shs, int64_t* counts, float* scale_out, float* mean_out) {
    float lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY};
    counts[0] = counts[1] = counts[2] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const float* row = block + i * n_attr;
        const float p[3] = {row[cols[0]], row[cols[1]], row[cols[2]]};
        float rp[3];
        im::rotate_position(p, rot, n_rot, rp);
        const int cls = im::classify(im::activate_opacity(row[cols[3]]), rp, opacity_threshold, has_area ? area : nullptr);
        cls_out[i] = cls;
        counts[cls == im::kSelected ? 0 : (cls == im::kUnselected ? 1 : 2)]++;
        if (cls == im::kSelected)
            for (int d = 0; d < 3; ++d) { lo[d] = fminf(lo[d], rp[d]); hi[d] = fmaxf(hi[d], rp[d]); }
    }
    if (counts[0] == 0) return 2;
    float mean[3], scale;
    const float max_diff = im::frame_of_bounds(lo, hi, mean, &scale);
    *scale_out = scale;
    for (int d = 0; d < 3; ++d) mean_out[d] = mean[d];
    if (!(max_diff > 0.0f)) return 3;
    int64_t n_sel = 0, n_unsel = 0;
    for (int64_t i = 0; i < n; ++i) {
        if (cls_out[i] == im::kDropped) continue;
        const float* row = block + i * n_attr;
        const int64_t dst = cls_out[i] == im::kSelected ? n_sel++ : counts[0] + n_unsel++;
        const float p[3] = {row[cols[0]], row[cols[1]], row[cols[2]]};
        const float ls[3] = {row[cols[4]], row[cols[5]], row[cols[6]]};
        const float q[4] = {row[cols[7]], row[cols[8]], row[cols[9]], row[cols[10]]};
        float c6[6];
        im::covariance(ls, q, c6);
        if (cls_out[i] == im::kSelected) {
            float rp[3], rc[6];
            im::rotate_position(p, rot, n_rot, rp);
            im::map_position(rp, mean, scale, z_shift, pos + 3 * dst);
            im::rotate_covariance(c6, rot, n_rot, rc);
            im::map_covariance(rc, scale, cov + 6 * dst);
        } else {
            for (int d = 0; d < 3; ++d) pos[3 * dst + d] = p[d];
            for (int d = 0; d < 6; ++d) cov[6 * dst + d] = c6[d];
        }
        opacity[dst] = im::activate_opacity(row[cols[3]]);
        for (int j = 0; j < K; ++j)
            for (int c = 0; c < 3; ++c)
                shs[(dst * K + j) * 3 + c] = row[cols[j == 0 ? 11 + c : 14 + c * (K - 1) + (j - 1)]];
    }
    return 0;
}
}
