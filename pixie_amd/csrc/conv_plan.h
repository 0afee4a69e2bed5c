// pixie_amd/csrc/conv_plan.h -- the launch plan of one convolution: WHAT pixie_conv3d_forward launches for a descriptor.
//
// conv_plan() is a pure host function of the descriptor's shape fields and of flags that say which optional operands are given.
// The launchers copy its geometry into the kernel arguments; every size query and diagnostic of include/pixie_hip.h reads the same
// plan, and so does the U-Net executor (unet_exec.hip), for its dry run and its real pass alike.  A new tile rule or kernel variant
// changes conv_plan() (conv3d_f16x3.hip) and the one variant table below.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/pixie_hip.h"

namespace pixie {

// The kernel instantiations <KS, MB, NB> of conv3d_f16x3_kernel, conv3d_f16x3_skip_kernel (the same launch with a folded 1x1x1 skip:
// conv_plan() can answer skip_foldable with every one of them), conv3d_exact_kernel and (with CK = 4 / 16 channels per LDS
// stage for KS = 3 / 1) the first-generation conv3d_mfma_kernel: MB blocks of 32 output channels x 4 waves x NB blocks of 32 voxels.
#define PX_CONV_VARIANTS(X) \
    X(3, 2, 4) X(3, 2, 2) X(3, 2, 1) X(3, 1, 4) X(3, 1, 2) X(3, 1, 1) X(1, 2, 4) X(1, 2, 2) X(1, 2, 1) X(1, 1, 4) X(1, 1, 2) X(1, 1, 1)

// What a launch is planned from.  The flags state what the caller has; the planner never looks at a pointer.
struct ConvShape {
    int c0 = 0, c1 = 0, c_out = 0, in_d = 0, in_h = 0, in_w = 0, ksize = 0, stride = 1, upsample = 0;
    int out_d = 0, out_h = 0, out_w = 0;     // odd-grid crop, 0 = none
    int skip_c0 = 0, skip_c1 = 0;            // channels a folded 1x1x1 skip convolution would read
    bool w16 = false;                        // f16x2-packed weights are given: the caller asks for the f16x3 path
    bool subpixel = false;                   // ... packed in sub-pixel form
    bool workspace = false;                  // a split-K workspace is (or would be) available
    bool skip = false;                       // a folded skip convolution rides along
    bool exact_v1 = false;                   // exact-fp32 descriptors go to the first-generation kernel (PIXIE_CONV_EXACT_V1)
};

enum ConvPath { CONV_NONE = 0, CONV_F16X3, CONV_F16X3_SUBPIXEL, CONV_EXACT_TILED, CONV_FIRST_GEN };
// why the shape does not allow the path the caller asked for (path == CONV_NONE)
enum ConvRefusal { CONV_OK = 0, CONV_BAD_SHAPE, CONV_BAD_STRIDE, CONV_BAD_CHANNELS, CONV_BAD_SUBPIXEL, CONV_BAD_LDS };

// where a launch leaves its partial statistics: n partials per channel, (sum, sum of squares) pairs; partial t of channel c lies
// at pair index c * cstride + t * tstride; f64: fp64 reduce segments (split-K), else the fp32 tile partials of the conv epilogue
struct ConvStatLayout { int n; long cstride, tstride; int f64; };

struct ConvPlan {
    ConvPath path = CONV_NONE; ConvRefusal refusal = CONV_OK;
    int KS = 0, MB = 0, NB = 0;              // the kernel entry (sub-pixel: conv3d_f16x3_subpixel_kernel<MB>)
    bool fullres = false;                    // ... under the symbol conv3d_f16x3_c64_fullres_kernel
    int slices = 1, chunks_per_slice = 0;    // split-K over the 16-channel chunks (chunks_per_slice: 0 unsplit)
    int OD = 0, OH = 0, OW = 0, coutp = 0;   // output dims (every path), c_out padded
    int ups = 0, LD = 0, LH = 0, LW = 0;     // the upsampling the kernel applies and the logical input dims (sub-pixel: the stored tensor)
    // tile and halo geometry of the tiled paths, as Conv16Args carries it
    int TX = 0, TY = 0, TZ = 0, lTX = 0, lTY = 0, tiles_x = 0, tiles_y = 0, tiles_z = 0, n_tiles = 0;
    int HX = 0, HY = 0, HZ = 0, HYX = 0, CS = 0; unsigned mHX = 0, mHYX = 0;
    int epi_lds = 0;                         // the launch reserves the transposing epilogue's LDS
    size_t lds_bytes = 0; dim3 grid;
    ConvStatLayout stats{0, 0, 0, 0};        // f16x3 paths
    int64_t stats_floats = 0;                // floats of d_out_stats (0 off the f16x3 paths)
    int64_t workspace_bytes = 0;             // bytes of d_workspace the split launch writes (0 unsplit)
    bool skip_foldable = false;              // this launch can take a folded skip convolution over skip_c0 + skip_c1 channels

    bool f16x3() const { return path == CONV_F16X3 || path == CONV_F16X3_SUBPIXEL; }
    bool tiled() const { return f16x3() || path == CONV_EXACT_TILED; }
};

// tile arithmetic of both launchers: the multiplier of the kernels' fast_div, ceil(log2 v), the largest power of two <= min(v, cap)
inline unsigned magic_of(int d) { return d <= 1 ? 0u : (unsigned)((0x100000000ull + (unsigned long long)d - 1) / (unsigned long long)d); }
inline int ilog2(int v) { int l = 0; while ((1 << l) < v) ++l; return l; }
inline int pow2_le(int v, int cap) { int p = 1; while (p * 2 <= v && p * 2 <= cap) p *= 2; return p; }

ConvPlan conv_plan(const ConvShape& s);
// the shape fields of a descriptor; flags from which of its optional pointers are set (and the environment, for exact_v1)
ConvShape conv_shape_of(const pixie_conv_desc* d);
bool conv_exact_v1();

// pixie_conv3d_forward's two tiled launchers (conv3d_f16x3.hip); p = conv_plan(conv_shape_of(d))
int conv3d_f16x3_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st);
int conv3d_exact_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st);

}  // namespace pixie
