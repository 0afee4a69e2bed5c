// pixie_amd/csrc/conv_stat_kernels.h -- the small kernels around the convolution launch: the statistics finalisers that add up what
// the conv epilogue (conv16_epilogue.h) or the split-K reduce left per tile / per segment, the two split-K reduces, and the |x|max
// of a tensor.  Launched from conv3d_f16x3.hip.  kReduceSeg, the voxels per reduce segment, is the planner's (conv_plan.h): it
// sizes the statistics buffer of a split launch.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_plan.h"
#include "launch_record.h"

namespace pixie {

// Where a producer left the partial statistics of its output: n partials per channel, (sum, sum of squares) pairs; partial t of
// channel c lies at pair index c * cstride + t * tstride.  The conv epilogues write stats[tile][coutp] in fp32, the split-K
// reduce writes stats[c][segment] in fp64.  n = 0: the channel's double[2] sums are already final.
struct StatParts { const void* p; int n; long cstride, tstride; int f64; };

// One workgroup (256 threads) adds the partials of channel c in fp64, in a fixed order: thread t takes partials t, t + 256, ...,
// then the 64-lane tree, then the four waves.  Every thread returns the totals; r is 8 doubles of LDS, free again on return.
__device__ inline void block_channel_sums(const StatParts& P, int c, double* r, double& o1, double& o2) {
    double s1 = 0.0, s2 = 0.0;
    for (int t = threadIdx.x; t < P.n; t += 256) {
        const size_t k = ((size_t)c * P.cstride + (size_t)t * P.tstride) * 2;
        if (P.f64) { const double2 v = *reinterpret_cast<const double2*>(static_cast<const double*>(P.p) + k); s1 += v.x; s2 += v.y; }
        else { const float2 v = *reinterpret_cast<const float2*>(static_cast<const float*>(P.p) + k); s1 += v.x; s2 += v.y; }
    }
    for (int off = 32; off > 0; off >>= 1) { s1 += __shfl_down(s1, off, 64); s2 += __shfl_down(s2, off, 64); }
    if ((threadIdx.x & 63) == 0) { r[2 * (threadIdx.x >> 6)] = s1; r[2 * (threadIdx.x >> 6) + 1] = s2; }
    __syncthreads();
    o1 = r[0] + r[2] + r[4] + r[6]; o2 = r[1] + r[3] + r[5] + r[7];
    __syncthreads();
}

// partial statistics -> sums[c][2] (fp64), one workgroup per channel
__global__ __launch_bounds__(256) void stats_finalize_kernel(StatParts P, double* __restrict__ sums) {
    const int c = blockIdx.x;
    __shared__ double r[8];
    double s1, s2;
    block_channel_sums(P, c, r, s1, s2);
    if (threadIdx.x == 0) { sums[2 * c] = s1; sums[2 * c + 1] = s2; }
}

// stats_finalize_kernel and norm_finalize_kernel (unet_ops.hip) in one launch: the producers' partials -> the double[2c] sums
// (kept: a later concatenation reads them again) AND the consumer's per-channel affine (a, b), same arithmetic as
// norm_finalize_kernel.  The statistics of th.cat([x0, x1]) are channels [0, c0) of part 0 and [c0, channels) of part 1; a part
// whose sums are final already has P.n = 0.  mode 0: one workgroup per channel; mode 1: one per group, which adds its channels
// in ascending order.  No workgroup needs another one's result.
__global__ __launch_bounds__(256) void stats_norm_finalize_kernel(StatParts P0, double* sums0, int c0, StatParts P1, double* sums1, int channels,
                                                                  double spatial, int mode, int groups, double eps,
                                                                  const float* __restrict__ weight, const float* __restrict__ bias,
                                                                  float* __restrict__ a, float* __restrict__ b) {
#include "conv_stat_norm_finalize.h"
}
// Grouped twin (launch_list.h): the same launch for two networks at once, blockIdx.z picks the argument set.  The members are the
// single form's parameters in order.
struct StatsNormFinalizeArgs {
    StatParts P0; double* sums0; int c0; StatParts P1; double* sums1; int channels; double spatial; int mode, groups; double eps;
    const float* weight; const float* bias; float* a; float* b;
};
__global__ __launch_bounds__(256) void stats_norm_finalize_group_kernel(Group2<StatsNormFinalizeArgs> G) {
    const StatsNormFinalizeArgs& A = G.a[blockIdx.z];
    const StatParts& P0 = A.P0; const StatParts& P1 = A.P1;
    double* sums0 = A.sums0; double* sums1 = A.sums1;
    const int c0 = A.c0, channels = A.channels, mode = A.mode, groups = A.groups;
    const double spatial = A.spatial, eps = A.eps;
    const float* weight = A.weight; const float* bias = A.bias; float* a = A.a; float* b = A.b;
#include "conv_stat_norm_finalize.h"
}

// out = sum_s partial[s] + bias (+ residual), slices added in a fixed order (deterministic split-K)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(const float* __restrict__ partial, int slices, long n_elems, long osp,
                                                            const float* __restrict__ bias, const float* residual, float* out) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_elems) return;
    float v = partial[i];
    for (int s = 1; s < slices; ++s) v += partial[(size_t)s * n_elems + i];
    if (bias) v += bias[i / osp];
    if (residual) v += residual[i];
    out[i] = v;
}

// The same reduce where the caller asked for the output's statistics: grid = (segments, c_out), a workgroup owns kReduceSeg
// consecutive voxels of ONE channel, so the bias is a workgroup constant, and while the stored values are in registers it takes
// their sum and sum of squares (fp64 from the first addition on) and their |x|max.  Every workgroup overwrites its own slot
// stats[c][segment][2] -- no floating-point atomics, nothing to zero -- and stats_norm_finalize_kernel adds the segments up.
// The output is bit-identical to splitk_reduce_kernel's: same slice order, then bias, then residual.
// |x|max: ONE atomicMax per workgroup, and none where the slot already holds a value as large.  The workgroups of these small
// layers all reach that point within microseconds of each other, and device-scope atomics on one address are served one after
// the other (measured: one atomic per wave made this kernel 119 us on average, against 13 us for splitk_reduce_kernel).
// VEC: osp % 4 == 0 and 16-byte aligned pointers, float4 accesses; otherwise strided scalars.
template <bool VEC>
__global__ __launch_bounds__(256) void splitk_reduce_stats_kernel(const float* __restrict__ partial, int slices, long n_elems, long osp,
                                                                  const float* __restrict__ bias, const float* residual, float* out,
                                                                  double* __restrict__ stats, unsigned* out_amax) {
#include "conv_stat_splitk_reduce.h"
}
// Grouped twin (launch_list.h): two networks' reduces of the same shape in one launch, blockIdx.z picks the argument set
struct SplitkReduceStatsArgs {
    const float* partial; int slices; long n_elems, osp; const float* bias; const float* residual; float* out; double* stats; unsigned* out_amax;
};
template <bool VEC>
__global__ __launch_bounds__(256) void splitk_reduce_stats_group_kernel(Group2<SplitkReduceStatsArgs> G) {
    const SplitkReduceStatsArgs& A = G.a[blockIdx.z];
    const float* partial = A.partial; const float* bias = A.bias; const float* residual = A.residual;
    const int slices = A.slices;
    const long n_elems = A.n_elems, osp = A.osp;
    float* out = A.out; double* stats = A.stats; unsigned* out_amax = A.out_amax;
#include "conv_stat_splitk_reduce.h"
}

// |x|max of a tensor as float bits (non-negative floats order like unsigned integers); caller zeroes the slot
__global__ __launch_bounds__(256) void amax_kernel(const float* __restrict__ x, long n, unsigned* __restrict__ slot) {
    float m = 0.0f;
    const long stride = (long)gridDim.x * 256 * 4;
    long i = ((long)blockIdx.x * 256 + threadIdx.x) * 4;
    if ((reinterpret_cast<size_t>(x) & 15) == 0) {
        for (; i + 3 < n; i += stride) {
            const float4 v = *reinterpret_cast<const float4*>(x + i);
            m = fmaxf(fmaxf(m, fabsf(v.x)), fmaxf(fabsf(v.y), fmaxf(fabsf(v.z), fabsf(v.w))));
        }
        for (long k = i; k < n && k < i + 4; ++k) m = fmaxf(m, fabsf(x[k]));
    } else {
        for (long k = (long)blockIdx.x * 256 + threadIdx.x; k < n; k += (long)gridDim.x * 256) m = fmaxf(m, fabsf(x[k]));
    }
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(slot, __float_as_uint(m));
}

}  // namespace pixie
