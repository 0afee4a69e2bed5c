// pixie_amd/csrc/conv_stat_kernels.h -- the small kernels around the convolution launch: the statistics finalisers that add up what
// the conv epilogue (conv16_epilogue.h) or the split-K reduce left per tile / per segment, the two split-K reduces, and the |x|max
// of a tensor.  Launched from conv3d_f16x3.hip.  kReduceSeg, the voxels per reduce segment, is the planner's (conv_plan.h): it
// sizes the statistics buffer of a split launch.
#pragma once
#include <hip/hip_runtime.h>

#include "conv_plan.h"

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
    __shared__ double r[8];
    const int cpg = mode == 0 ? 1 : channels / groups;
    const int first = blockIdx.x * cpg;
    double s1 = 0.0, s2 = 0.0;
    for (int k = first; k < first + cpg; ++k) {
        const bool in0 = k < c0;
        const StatParts& P = in0 ? P0 : P1;
        double* sums = in0 ? sums0 : sums1;
        const int kc = in0 ? k : k - c0;
        double t1, t2;
        if (P.n > 0) {
            block_channel_sums(P, kc, r, t1, t2);
            if (threadIdx.x == 0) { sums[2 * kc] = t1; sums[2 * kc + 1] = t2; }
        } else {
            t1 = sums[2 * kc]; t2 = sums[2 * kc + 1];
        }
        s1 += t1; s2 += t2;
    }
    const double cnt = mode == 0 ? spatial : spatial * cpg;
    const double mean = s1 / cnt;
    double var = s2 / cnt - mean * mean;
    if (var < 0.0) var = 0.0;
    const double rstd = 1.0 / sqrt(var + eps);
    for (int k = first + threadIdx.x; k < first + cpg; k += 256) {
        if (mode == 0) {
            a[k] = (float)rstd;
            b[k] = (float)(-mean * rstd);
        } else {
            const double w = weight ? (double)weight[k] : 1.0;
            const double bb = bias ? (double)bias[k] : 0.0;
            a[k] = (float)(rstd * w);
            b[k] = (float)(bb - mean * rstd * w);
        }
    }
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
    const int c = blockIdx.y;
    const long seg0 = (long)blockIdx.x * kReduceSeg;
    const size_t base = (size_t)c * osp;
    const float bv = bias ? bias[c] : 0.0f;
    double s1 = 0.0, s2 = 0.0;
    float mx = 0.0f;
    if (VEC) {
#pragma unroll
        for (int k = 0; k < kReduceSeg / 1024; ++k) {
            const long j = seg0 + k * 1024 + (long)threadIdx.x * 4;
            if (j < osp) {
                const size_t i = base + j;
                float4 v = *reinterpret_cast<const float4*>(partial + i);
                for (int s = 1; s < slices; ++s) {
                    const float4 q = *reinterpret_cast<const float4*>(partial + (size_t)s * n_elems + i);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                if (bias) { v.x += bv; v.y += bv; v.z += bv; v.w += bv; }
                if (residual) {
                    const float4 q = *reinterpret_cast<const float4*>(residual + i);
                    v.x += q.x; v.y += q.y; v.z += q.z; v.w += q.w;
                }
                *reinterpret_cast<float4*>(out + i) = v;
                const double x = v.x, y = v.y, z = v.z, w = v.w;
                s1 += (x + y) + (z + w);
                s2 += (x * x + y * y) + (z * z + w * w);
                mx = fmaxf(fmaxf(mx, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
            }
        }
    } else {
#pragma unroll 4
        for (int k = 0; k < kReduceSeg / 256; ++k) {
            const long j = seg0 + k * 256 + threadIdx.x;
            if (j < osp) {
                const size_t i = base + j;
                float v = partial[i];
                for (int s = 1; s < slices; ++s) v += partial[(size_t)s * n_elems + i];
                if (bias) v += bv;
                if (residual) v += residual[i];
                out[i] = v;
                const double x = v;
                s1 += x; s2 += x * x; mx = fmaxf(mx, fabsf(v));
            }
        }
    }
    for (int off = 32; off > 0; off >>= 1) {
        s1 += __shfl_down(s1, off, 64);
        s2 += __shfl_down(s2, off, 64);
        mx = fmaxf(mx, __shfl_down(mx, off, 64));
    }
    __shared__ double r[8];
    __shared__ float rmx[4];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    if (lane == 0) { r[2 * wave] = s1; r[2 * wave + 1] = s2; rmx[wave] = mx; }
    __syncthreads();
    if (threadIdx.x == 0) {
        double* dst = stats + ((size_t)c * gridDim.x + blockIdx.x) * 2;
        dst[0] = r[0] + r[2] + r[4] + r[6];
        dst[1] = r[1] + r[3] + r[5] + r[7];
        const unsigned m = __float_as_uint(fmaxf(fmaxf(rmx[0], rmx[1]), fmaxf(rmx[2], rmx[3])));
        // the slot only grows: a stale read can only be too small, and then costs the atomic it would have cost anyway
        if (out_amax && m > __hip_atomic_load(out_amax, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) atomicMax(out_amax, m);
    }
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
