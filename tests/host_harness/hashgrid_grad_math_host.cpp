// tests/host_harness/hashgrid_grad_math_host.cpp -- pixie_amd/csrc/hashgrid_grad_math.h compiled for the host (g++
// -ffp-contract=off), for tests/test_hashgrid_grad_math.py: the same lines the table-gradient kernels run.
#include "../../pixie_amd/csrc/hashgrid_grad_math.h"

using namespace pixie;

extern "C" {

int hh_hgg_state(uint32_t bits) { return hgg::state_of(bits); }
int hh_hgg_pow2_above(uint32_t bits) { return hgg::pow2_above(bits); }
int hh_hgg_shift(uint32_t bits, int64_t n) { return hgg::shift_of(bits, n); }
int hh_hgg_ceil_log2(uint64_t v) { return hgg::ceil_log2(v); }
uint32_t hh_hgg_magnitude_bits(float x) { return hgg::magnitude_bits(x); }
int64_t hh_hgg_quantise(float c, int s) { return hgg::quantise(c, s); }
float hh_hgg_finalise(int64_t acc, int s) { return hgg::finalise(acc, s); }

// the accumulator of `count` contributions in the order given (two's complement wrap-around, as the device's integer atomic adds)
int64_t hh_hgg_sum(const float* c, int64_t count, int s) {
    uint64_t acc = 0;
    for (int64_t i = 0; i < count; ++i) acc += (uint64_t)hgg::quantise(c[i], s);
    return (int64_t)acc;
}

}  // extern "C"
