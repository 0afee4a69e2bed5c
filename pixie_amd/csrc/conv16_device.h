// pixie_amd/csrc/conv16_device.h -- what every piece of the f16x3 convolution's device code shares: the vector typedefs, the packed
// weights' header size, the kernel argument block Conv16Args (filled by conv16_args() and the two launchers in conv3d_f16x3.hip
// from the launch plan of conv_plan.h) and the small device functions of the tiled body (conv16_body.h and its fragments) and of
// the weight packers (conv_pack_kernels.h).  An ordinary header; conv3d_f16x3.hip is the one translation unit that includes it.
#pragma once
#include <hip/hip_runtime.h>

namespace pixie {

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

constexpr int kW16HeaderU4 = 4;  // 64-byte header in front of the packed planes: [0].x = bits of 1/s_w

struct Conv16Args {
    const float* in0; const float* in1;
    int c0, cin;
    int ID, IH, IW;          // stored input dims
    int LD, LH, LW;          // logical input dims (after optional nearest x2)
    int ups;
    int stride;              // 1, or 2 (3^3 Downsample convs: the LDS tile then holds every input voxel, the B reads skip one)
    int OD, OH, OW;
    const float* pro_a; const float* pro_b; const float* gamma; const float* beta;
    int act;
    const uint4* w16;        // packed weights (header + hi planes + lo planes)
    const float* wf;         // EXACT variant: fp32 weights [tap][c_in][c_out padded] (pixie_conv_pack_weights) instead of w16
    const float* bias;
    int cout, coutp;
    const float* residual; float* out;
    const unsigned* amax0; const unsigned* amax1;   // device |x|max of in0 / in1 as float bits, or null
    float in_bound;                                  // host bound on |prologue(x)| when amax0 is null
    int TX, TY, TZ, lTX, lTY;
    int tiles_x, tiles_y, tiles_z, n_tiles;
    int HX, HY, HZ, HYX, CS;
    unsigned mHX, mHYX;
    float* stats; unsigned* out_amax;   // epilogue statistics (conv16_epilogue.h), or null
    float* partial; int chunks_per_slice;   // split-K: blockIdx.z handles chunks [z*cps, (z+1)*cps) and writes partial[z]
    int epi_lds;             // the launch reserved enough LDS for the transposing epilogue (4 x 32 x (32 NB + 4) + 256 MB floats)
    // Folded 1x1x1 skip convolution (MyResBlock.skip_connection, diffusion_network.py:691,705): after the main chunks the
    // accumulators are rescaled (an exact power of two) and sk_cin more channels of the RAW tensors sk_in0 | sk_in1 are
    // accumulated through the centre tap only, with their own packed weights, input scale and bias.
    const float* sk_in0; const float* sk_in1;
    int sk_c0, sk_cin;
    const uint4* sk_w16; const float* sk_bias;
    const unsigned* sk_amax0; const unsigned* sk_amax1;
};

__device__ __forceinline__ int fast_div16(int n, int d, unsigned magic) {
    return (d == 1) ? n : (int)__umulhi((unsigned)n, magic);
}
__device__ __forceinline__ float act16(float t, int act) {
    if (act == 1) return t > 0.0f ? t : 0.02f * t;
    if (act == 2) return t / (1.0f + __expf(-t));
    return t;
}
// The same values for the f16x3 staging (the exact-fp32 body keeps act16).  fmaxf(t, 0.02 t) is the LeakyReLU select bit for bit, for
// +-0, +-inf and NaN too (t > 0: t > 0.02 t; t < 0: 0.02 t > t; at +-0 both operands are the same zero): one v_max_f32 for a compare
// and a select.  The SiLU division stays IEEE: a denominator of +inf (t below about -88.7) gives -0.
__device__ __forceinline__ float act16_staged(float t, int act) {
    if (act == 1) return fmaxf(t, 0.02f * t);
    if (act == 2) return t / (1.0f + __expf(-t));
    return t;
}
// power-of-two scale that maps |x| <= bound to below 2^15 (fp16 max is 65504): s = 2^(14 - floor(log2 bound))
__device__ __forceinline__ int scale_exponent(float bound) {
    const unsigned bits = __float_as_uint(bound);
    const int eb = (int)((bits >> 23) & 0xffu) - 127;
    if (!(bound > 0.0f) || eb > 100) return 0;   // zero tensor, NaN or inf: any scale will do
    int e = 14 - eb;
    return e > 100 ? 100 : (e < -100 ? -100 : e);
}
__device__ __forceinline__ float pow2i(int e) { return __uint_as_float((unsigned)(e + 127) << 23); }

}  // namespace pixie
