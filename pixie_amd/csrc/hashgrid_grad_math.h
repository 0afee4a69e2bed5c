// pixie_amd/csrc/hashgrid_grad_math.h -- the fixed-point rule of the hash table's gradient (field_query_backward.hip), as
// __host__ __device__ functions, so that tests/host_harness/hashgrid_grad_math_host.cpp runs the same lines on the CPU against
// Python integers (tests/test_hashgrid_grad_math.py).
//
// The table gradient is a scatter of n * levels * 8 float32 contributions c = w_corner * dX[column] per feature.  Each is added to an
// int64 accumulator as llrint(c * 2^s); the accumulator becomes float32(double(acc) * 2^-s).  The shift s is a pure function of the
// bits of M = max |dX_grid| over the call and of n:
//   2^e > M, e the smallest such integer (M = 2^k gives e = k + 1; denormals count their leading bit)
//   s = 62 - e - ceil(log2(8 n))
// A corner weight is a product of three factors in [0, 1], so |c| <= M < 2^e and |c * 2^s| < 2^(62 - ceil(log2(8 n))): 8 n of them
// (every (point, level) touches a row at most 8 times) sum to less than 2^62 in magnitude.  c * 2^s is a float32 times a power of
// two below 2^62: exact, unless it falls under the denormal range, where it rounds to an integer anyway.  Integer addition is
// associative, M is a maximum: the sum does not depend on the order of the points.
// M == 0: nothing is scattered (state 1).  M not finite (Inf or NaN bits): no float is converted, the gradient is NaN (state 2).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HGG_HD __host__ __device__ inline
#else
#define HGG_HD inline
#endif

namespace pixie {
namespace hgg {

constexpr int64_t kMaxPoints = (int64_t)1 << 24;
enum State { kNormal = 0, kZero = 1, kNonFinite = 2 };

// |x| as the integer whose unsigned order is the order of magnitudes; every NaN lies above Inf
HGG_HD uint32_t magnitude_bits(float x) {
    union { float f; uint32_t u; } v;
    v.f = x;
    return v.u & 0x7fffffffu;
}

HGG_HD int state_of(uint32_t max_bits) { return max_bits == 0u ? kZero : (max_bits >= 0x7f800000u ? kNonFinite : kNormal); }

HGG_HD int ceil_log2(uint64_t v) {            // v >= 1
    int b = 0;
    while (b < 63 && ((uint64_t)1 << b) < v) ++b;
    return b;
}

// e with 2^(e - 1) <= M < 2^e, for the bits of a finite M > 0
HGG_HD int pow2_above(uint32_t max_bits) {
    const int biased = (int)(max_bits >> 23);
    if (biased > 0) return biased - 127 + 1;
    int top = 22;                               // denormal: M = mantissa * 2^-149
    while (!((max_bits >> top) & 1u)) --top;
    return top - 149 + 1;
}

HGG_HD int shift_of(uint32_t max_bits, int64_t n) { return 62 - pow2_above(max_bits) - ceil_log2(8u * (uint64_t)n); }

HGG_HD int64_t quantise(float c, int s) { return (int64_t)llrintf(ldexpf(c, s)); }

HGG_HD float finalise(int64_t acc, int s) { return (float)ldexp((double)acc, -s); }

}  // namespace hgg
}  // namespace pixie
