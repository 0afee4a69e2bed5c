// pixie_amd/csrc/conv_stat_splitk_reduce.h -- FRAGMENT of splitk_reduce_stats_kernel<VEC> and of its grouped twin
// (conv_stat_kernels.h), included inside each as its statements, like conv_stat_norm_finalize.h and for the same reason: behind a
// __forceinline__ function the single form compiles to other code than it had.  No include guard: included once per kernel.
//   names read:   VEC, partial, slices, n_elems, osp, bias, residual, out, stats, out_amax
//   writes:       out, stats[c][segment][2], *out_amax; LDS: r[8], rmx[4]
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
