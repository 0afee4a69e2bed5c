// pixie_amd/csrc/conv_pack_kernels.h -- the weight packers of the f16x3 convolution: fp32 weights -> 64-byte header + fp16 hi planes +
// fp16 lo planes in the layout the tap loop (conv16_taps.h) reads, in the plain form ([tap][c_in/8][c_out padded]) and in the
// sub-pixel form (pre-summed 2 x 2 x 2 taps per output parity).  Launched from conv3d_f16x3.hip.
#pragma once
#include <hip/hip_runtime.h>

#include "conv16_device.h"

namespace pixie {

// (c_out, c_in, taps) fp32 -> header + hi planes + lo planes of [tap][c_in/8][c_out_padded] x (8 x fp16)
__global__ void pack_weights_f16x2_kernel(const float* __restrict__ src, uint4* __restrict__ dst, int cout, int cin, int taps,
                                          int coutp, const unsigned* __restrict__ amax_bits) {
    const int KG = cin >> 3;
    const long total = (long)taps * KG * coutp;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = scale_exponent(__uint_as_float(*amax_bits));
    if (i == 0) dst[0] = make_uint4(__float_as_uint(pow2i(-e)), (unsigned)cout, (unsigned)cin, (unsigned)taps);
    if (i >= total) return;
    const float s = pow2i(e);
    const int co = (int)(i % coutp);
    const long row = i / coutp;
    const int kg = (int)(row % KG);
    const int tap = (int)(row / KG);
    f16x8 vh, vl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float w = 0.0f;
        if (co < cout) w = src[((long)co * cin + kg * 8 + j) * taps + tap] * s;
        const _Float16 h = (_Float16)w;
        vh[j] = h;
        vl[j] = (_Float16)(w - (float)h);
    }
    dst[kW16HeaderU4 + i] = __builtin_bit_cast(uint4, vh);
    dst[kW16HeaderU4 + total + i] = __builtin_bit_cast(uint4, vl);
}

// Sub-pixel weights of a 3^3 convolution behind a nearest x2 upsampling.  Per axis, output parity p and effective tap e
// sum the original taps  p=0: e=0 {0}, e=1 {1,2};  p=1: e=0 {0,1}, e=1 {2}  (tap index 0..2 = offset -1..1), in fp32, in
// ascending (dz, dy, dx) order.  par = (pz*2 + py)*2 + px, tap = (ez*2 + ey)*2 + ex.
__device__ __forceinline__ float subpixel_weight(const float* __restrict__ w27, int par, int tap) {
    int lo[3], hi[3];
#pragma unroll
    for (int ax = 0; ax < 3; ++ax) {   // ax 0 = z
        const int p = (par >> (2 - ax)) & 1, e = (tap >> (2 - ax)) & 1;
        lo[ax] = e ? (p ? 2 : 1) : 0;
        hi[ax] = e ? 2 : (p ? 1 : 0);
    }
    float sum = 0.0f;
    for (int dz = lo[0]; dz <= hi[0]; ++dz)
        for (int dy = lo[1]; dy <= hi[1]; ++dy)
            for (int dx = lo[2]; dx <= hi[2]; ++dx) sum += w27[(dz * 3 + dy) * 3 + dx];
    return sum;
}
// |w|max of the summed weights (float bits, atomicMax; caller zeroes the slot): one thread per (c_out, c_in) pair
__global__ __launch_bounds__(256) void subpixel_amax_kernel(const float* __restrict__ src, long pairs, unsigned* __restrict__ slot) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    float m = 0.0f;
    if (i < pairs)
        for (int pt = 0; pt < 64; ++pt) m = fmaxf(m, fabsf(subpixel_weight(src + i * 27, pt >> 3, pt & 7)));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_down(m, off, 64));
    if ((threadIdx.x & 63) == 0 && m > 0.0f) atomicMax(slot, __float_as_uint(m));
}
// (c_out, c_in, 27) fp32 -> header + hi planes + lo planes of [parity 8][tap 8][c_in/8][c_out_padded] x (8 x fp16); the
// split is pack_weights_f16x2_kernel's, applied to the summed weights
__global__ void pack_weights_subpixel_kernel(const float* __restrict__ src, uint4* __restrict__ dst, int cout, int cin, int coutp,
                                             const unsigned* __restrict__ amax_bits) {
    const int KG = cin >> 3;
    const long total = 64L * KG * coutp;
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    const int e = scale_exponent(__uint_as_float(*amax_bits));
    if (i == 0) dst[0] = make_uint4(__float_as_uint(pow2i(-e)), (unsigned)cout, (unsigned)cin, 64u);
    if (i >= total) return;
    const float s = pow2i(e);
    const int co = (int)(i % coutp);
    const long row = i / coutp;
    const int kg = (int)(row % KG);
    const int pt = (int)(row / KG);
    f16x8 vh, vl;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        float w = 0.0f;
        if (co < cout) w = subpixel_weight(src + ((long)co * cin + kg * 8 + j) * 27, pt >> 3, pt & 7) * s;
        const _Float16 h = (_Float16)w;
        vh[j] = h;
        vl[j] = (_Float16)(w - (float)h);
    }
    dst[kW16HeaderU4 + i] = __builtin_bit_cast(uint4, vh);
    dst[kW16HeaderU4 + total + i] = __builtin_bit_cast(uint4, vl);
}

}  // namespace pixie
