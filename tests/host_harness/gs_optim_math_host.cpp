// tests/host_harness/gs_optim_math_host.cpp -- pixie_amd/csrc/gs_optim_math.h compiled for the host (g++ -ffp-contract=off), so that
// tests/test_gs_optim_math.py can run the arithmetic of the kernels in gs_optim.hip on the CPU: the Adam element update, the
// densification decisions and the values of split children.
#include <cstdint>

#include "../../pixie_amd/csrc/gs_optim_math.h"

namespace gm = pixie::gso;

extern "C" {

// one Adam step over n elements, the scalars prepared as pixie_gs_adam_step prepares them
int hh_gs_adam(int64_t n, float* p, const float* g, float* m, float* v, double beta1, double beta2, double eps, double step_size,
               double bc2_sqrt) {
    const float w1 = (float)(1.0 - beta1), b2 = (float)beta2, w2 = (float)(1.0 - beta2), e = (float)eps;
    for (int64_t i = 0; i < n; ++i) gm::adam_element(p[i], g[i], m[i], v[i], w1, b2, w2, e, (float)step_size, (float)bc2_sqrt);
    return 0;
}

// flags[i] = classify(...) with the thresholds rounded as thresholds_of() in gs_optim.hip rounds them
int hh_gs_classify(int64_t n, const float* accum, const float* denom, const float* scaling, const float* opacity, double max_grad,
                   double min_opacity, double extent, double percent_dense, int has_max_screen_size, int32_t* flags) {
    for (int64_t i = 0; i < n; ++i)
        flags[i] = gm::classify(accum[i], denom[i], scaling + 3 * i, opacity[i], (float)max_grad, (float)(percent_dense * extent),
                                (float)min_opacity, has_max_screen_size, (float)(0.1 * extent));
    return 0;
}

// the computed fields of one split child per row
int hh_gs_split(int64_t n, const float* xyz, const float* scaling, const float* rotation, const float* z, float* out_xyz,
                float* out_scaling) {
    for (int64_t i = 0; i < n; ++i) {
        gm::split_position(xyz + 3 * i, scaling + 3 * i, rotation + 4 * i, z + 3 * i, out_xyz + 3 * i);
        gm::split_scaling(scaling + 3 * i, out_scaling + 3 * i);
    }
    return 0;
}

float hh_gs_stats_norm2(float gx, float gy) { return gm::stats_norm2(gx, gy); }

}  // extern "C"
