// pixie_amd/csrc/wave_order.h -- fixed-order sums and scans over one 64-lane wave, shared by the ray kernels (ray_render.hip,
// ray_sample.hip).  Every result depends on the lanes' values alone, never on the launch geometry.
#pragma once
#include <hip/hip_runtime.h>

namespace pixie {
namespace {

// every lane gets the same bits: at each step both partners add the same two values
__device__ inline float wave_sum(float v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = v + __shfl_xor(v, m, 64);
    return v;
}
__device__ inline int wave_min(int v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
        const int o = __shfl_xor(v, m, 64);
        v = o < v ? o : v;
    }
    return v;
}
// sum of the lanes below (Hillis-Steele over distances 1, 2, .. 32)
__device__ inline float wave_exclusive_prefix(float v, int lane) {
    float inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_up(inc, d, 64);
        if (lane >= d) inc = o + inc;
    }
    const float below = __shfl_up(inc, 1, 64);
    return lane == 0 ? 0.0f : below;
}
// sum of the lanes above
__device__ inline float wave_exclusive_suffix(float v, int lane) {
    float inc = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const float o = __shfl_down(inc, d, 64);
        if (lane + d < 64) inc = inc + o;
    }
    const float above = __shfl_down(inc, 1, 64);
    return lane == 63 ? 0.0f : above;
}

}  // namespace
}  // namespace pixie
