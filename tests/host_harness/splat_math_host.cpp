// tests/host_harness/splat_math_host.cpp -- compiles pixie_amd/csrc/splat_math.h for the HOST so that CPU-only tests can check
// the splat decomposition (covariance -> log-scales, quaternion) before any GPU run.
// Test infrastructure only: the product never executes this.
#include "../../pixie_amd/csrc/splat_math.h"
extern "C" {
void hh_splat_from_cov(int n, const float* cov, float* log_scale, float* quat) {
    for (int p = 0; p < n; ++p) pixie::splat::splat_from_cov(cov + 6 * p, log_scale + 3 * p, quat + 4 * p);
}
}
