// pixie_amd/csrc/unet_ops_internal.h -- what unet_ops.hip offers the plan walk (unet_walk.h) beside the entry points of
// include/pixie_hip.h: the launches of pixie_channel_stats / pixie_norm_finalize without their set-up work.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

namespace pixie {

// the launch of pixie_channel_stats for a d_sums the caller has already zeroed
int channel_stats_prezeroed(const float* d_x, int channels, int64_t spatial, double* d_sums, uint32_t* d_amax, hipStream_t st);
// pixie_norm_finalize over the channel concatenation of two tensors' statistics (no copy of either)
int norm_finalize_cat(const double* d_sums0, int c0, const double* d_sums1, int c1, int64_t spatial, int mode, int groups, double eps,
                      const float* d_weight, const float* d_bias, float* d_a, float* d_b, hipStream_t st);

}  // namespace pixie
