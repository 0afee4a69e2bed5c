// pixie_amd/csrc/conv3d_f16x3.hip -- the U-Net's 3D convolutions on the gfx950 f16 matrix cores at fp32-grade
// accuracy ("f16x3": every fp32 operand is split into two fp16 halves and three MFMAs replace one).
//
// Why: the exact-fp32 MFMA (v_mfma_f32_32x32x2_f32, conv3d_mfma.hip) runs at the fp32 vector rate, 157 TFLOP/s;
// v_mfma_f32_32x32x16_f16 runs at 2.5 PFLOP/s.  With  x*s = hi + lo  (hi = fp16(x*s), lo = fp16(x*s - hi), s a
// power of two that places the tensor just below the fp16 range, so hi+lo carries 22 significant bits),
//     w.x  ~  ( w_hi.x_hi + w_hi.x_lo + w_lo.x_hi ) / (s_w s_x)
// drops only the lo.lo term (2^-22 relative) and accumulates in fp32 inside the MFMA: three f16 MFMAs per
// fp32-equivalent product = 833 TFLOP/s of algorithmic peak, 5.3x the exact-fp32 pipe, at 2-3e-7 relative error
// per product (fp32's own is 6e-8).  The U-Net parity target (<= 1e-4 rel-L2 vs the fp32 reference) is kept with
// >100x margin; tests/test_unet_hip.py measures it.
//
// Replaces the same reference ops as conv3d_mfma.hip (WG/models/module/diffusion_network.py conv_nd at
// :679,:683,:691,:762,:58,:206,:208,:872, FeatureProjector :570-583) for stride-1 layers whose channel counts are
// multiples of 16 (stride 2 for the 3^3 Downsample convs); everything else (tiny test networks) stays on the exact-fp32 kernel.
//
// Formulation: Out[co][v] = sum_{tap,ci} W[tap][ci][co] X[ci][v+tap], implicit GEMM with M = c_out (A operand),
// N = voxels (B operand, 32 x-contiguous voxels per MFMA column block), K = taps*c_in walked tap by tap in steps
// of 16 channels (one MFMA K).  Workgroup = 4 waves, each MB*32 c_out x NB*32 voxels.
//   B: per 16-channel chunk the halo'd voxel tile is staged once in LDS as fp16 hi/lo planes laid out
//      [k-group of 8 channels][voxel] x 16 B, so a wave's B fragment is one conflict-free ds_read_b128 and the
//      same tile serves all 27 taps.  Prologue (norm affine, spatial LayerNorm affine, activation, zero padding
//      AFTER the activation, nearest x2 upsampling, channel concat) is applied on the way in, as in the fp32 kernel.
//   A: weights are pre-split and pre-swizzled on the device (conv_pack_kernels.h) into [tap][k-group][c_out] x 16 B
//      hi/lo planes; every wave reads its A fragments straight from L2 (two coalesced 512 B segments per load;
//      the whole 64->64 3^3 layer is 442 KB), so LDS holds activations only and two workgroups fit per CU.
//
// File map.  This file is the one translation unit; it keeps the kernel tables, the two launchers and the C API, and includes,
// in the order of the code object:
//   conv_plan.h          (pure host)  ConvShape -> ConvPlan: path, kernel entry, tile, split-K, LDS and buffer sizes; the pair form's
//                                     LDS rule; what the diagnostic queries answer.  g++-compiled for tests/test_conv_plan_host.py
//   conv_launch.h        declarations of what this file defines for conv3d_mfma.hip and unet_exec.hip: conv_shape_of, conv_exact_v1
//                        and the launchers conv3d_f16x3_forward, conv3d_exact_forward
//   conv16_device.h      typedefs, Conv16Args, fast_div16, act16, act16_staged, scale_exponent, pow2i
//   conv16_body.h        conv3d_f16x3_body: geometry, scale, accumulators, the chunk loop; the six __global__ entry points.
//                        It includes, inside the body, the fragments conv16_stage.h (stage_chunk), conv16_taps.h (mfma_chunk),
//                        conv16_skip.h (the folded 1x1x1 skip) and conv16_epilogue.h, each with its contract at its top
//   conv_stat_kernels.h  statistics finalisers, the split-K reduces, amax_kernel
//   conv_pack_kernels.h  the weight packers (plain and sub-pixel)
#include <hip/hip_runtime.h>

#include <cstdlib>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "conv_plan.h"
#include "conv_launch.h"
#include "launch_record.h"
#include "conv16_device.h"
#include "conv16_body.h"
#include "conv_stat_kernels.h"
#include "conv_pack_kernels.h"

namespace pixie {

bool conv_exact_v1() { return getenv("PIXIE_CONV_EXACT_V1") != nullptr; }

// the shape fields of a descriptor; flags from which of its optional pointers are set (and the environment, for exact_v1)
ConvShape conv_shape_of(const pixie_conv_desc* d) {
    ConvShape s;
    s.c0 = d->c0; s.c1 = d->c1; s.c_out = d->c_out;
    s.in_d = d->in_d; s.in_h = d->in_h; s.in_w = d->in_w;
    s.ksize = d->ksize; s.stride = d->stride; s.upsample = d->upsample;
    s.out_d = d->out_d; s.out_h = d->out_h; s.out_w = d->out_w;
    s.skip_c0 = d->skip_c0; s.skip_c1 = d->skip_c1;
    s.w16 = d->d_w16 != nullptr; s.subpixel = d->w16_subpixel != 0; s.workspace = d->d_workspace != nullptr; s.skip = d->d_skip_w16 != nullptr;
    s.exact_v1 = conv_exact_v1();
    return s;
}

// the kernel of a tiled plan: one table for the f16x3 and the exact instantiations
using ConvKernel = void (*)(Conv16Args);
// skip: the descriptor carries a folded skip convolution (f16x3 path, plan.skip_foldable) whose first part has skip_c0 channels
static ConvKernel conv16_kernel(const ConvPlan& p, bool skip = false, int skip_c0 = 0) {
    if (p.path == CONV_F16X3_SUBPIXEL) return p.MB == 2 ? conv3d_f16x3_subpixel_kernel<2> : conv3d_f16x3_subpixel_kernel<1>;
    if (p.fullres) return conv3d_f16x3_c64_fullres_kernel;
#define PX_CONV16_PICK(KS_, MB_, NB_)                                                                \
    if (p.KS == KS_ && p.MB == MB_ && p.NB == NB_)                                                   \
        return p.path == CONV_EXACT_TILED ? conv3d_exact_kernel<KS_, MB_, NB_>                       \
                                          : (!skip ? conv3d_f16x3_kernel<KS_, MB_, NB_>                                \
                                                   : ((skip_c0 & 8) ? conv3d_f16x3_skip_kernel<KS_, MB_, NB_, true> : conv3d_f16x3_skip_kernel<KS_, MB_, NB_, false>));
    PX_CONV_VARIANTS(PX_CONV16_PICK)
#undef PX_CONV16_PICK
    return nullptr;
}

// The grouped twin of conv16_kernel()'s answer (conv16_body.h), null where the launch has none.  The table holds the instantiations
// the shipped networks launch below full resolution whose grouped launch, measured there against two single launches, is not
// slower by more than 2 % (profiles/unet_pair_ab_ms_per_step.txt): <3,2,4>, sub-pixel <2>, <1,2,2>, <1,2,1>.  Measured and taken
// out: <3,2,2> (+6 % and +10 % at its two shapes), <3,2,1> (+6 % to +14 % at three of four), <1,2,4> (+13 % at the 32^3 level),
// the folded-skip form of <3,2,4> (+1.2 % in one trace, +3.0 % in the next).  Never in it: the 32-channel-block instantiations
// (MB = 1), which those networks do not launch there (<3,1,4> would also lose a wave of occupancy to its twin), the 8-wave pair
// form, the exact-fp32 kernels.  A launch without a twin stays two launches.
using ConvGroupKernel = void (*)(Group2<Conv16Args>);
template <int KS, int MB, int NB> static ConvGroupKernel conv16_group_pick() {
    if constexpr ((KS == 3 && MB == 2 && NB == 4) || (KS == 1 && MB == 2 && (NB == 2 || NB == 1))) return conv3d_f16x3_group_kernel<KS, MB, NB>;
    else return nullptr;
}
static ConvGroupKernel conv16_group_kernel(const ConvPlan& p, bool skip = false) {
    if (p.path == CONV_F16X3_SUBPIXEL) return p.MB == 2 ? conv3d_f16x3_subpixel_group_kernel<2> : nullptr;
    if (p.fullres || p.path == CONV_EXACT_TILED || skip) return nullptr;
#define PX_CONV16_PICK(KS_, MB_, NB_)                \
    if (p.KS == KS_ && p.MB == MB_ && p.NB == NB_) return conv16_group_pick<KS_, MB_, NB_>();
    PX_CONV_VARIANTS(PX_CONV16_PICK)
#undef PX_CONV16_PICK
    return nullptr;
}

// The pair form of a planned launch: conv_pair_lds_bytes() (conv_plan.h) decides it from the plan; returns the launch's dynamic LDS
// bytes, 0 = the launch keeps the 4-wave kernel.
#ifdef PIXIE_DIAG
static int g_conv_keep_four_wave = 0;   // diagnostic switch (pixie_conv_kernel_variant with a null descriptor)
#endif
static size_t conv_pair_lds(const ConvPlan& p, bool skip) {
#ifdef PIXIE_DIAG
    if (g_conv_keep_four_wave) return 0;
#endif
    return conv_pair_lds_bytes(p, skip);
}
static ConvKernel conv16_pair_kernel(const ConvPlan& p) {
#define PX_CONV16_PAIR(KS_, NB_) \
    if (p.KS == KS_ && p.NB == NB_) return conv3d_f16x3_pair_kernel<KS_, NB_>;
    PX_CONV16_PAIR(3, 4) PX_CONV16_PAIR(1, 4)
#undef PX_CONV16_PAIR
    return nullptr;
}

static int launch(ConvKernel kern, const ConvPlan& p, const Conv16Args& a, hipStream_t st, size_t pair_lds = 0, ConvGroupKernel twin = nullptr) {
    PX_REQUIRE(kern != nullptr, "conv: no kernel variant for ksize=%d MB=%d NB=%d", p.KS, p.MB, p.NB);
    PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(kern)));
    if (twin && launch_recorder()) PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(twin)));
    if (pair_lds) px_launch(kern, dim3(p.grid_x, p.grid_y / 2, 1), dim3(512), pair_lds, st, a);
    else if (twin) px_launch_grouped(kern, twin, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(256), p.lds_bytes, st, a);
    else px_launch(kern, dim3(p.grid_x, p.grid_y, p.grid_z), dim3(256), p.lds_bytes, st, a);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

// the plan's geometry and the operands both tiled paths share
static Conv16Args conv16_args(const pixie_conv_desc* d, const ConvPlan& p) {
    Conv16Args a{};
    a.in0 = d->d_in0; a.in1 = d->d_in1; a.c0 = d->c0; a.cin = d->c0 + d->c1;
    a.ID = d->in_d; a.IH = d->in_h; a.IW = d->in_w;
    a.LD = p.LD; a.LH = p.LH; a.LW = p.LW; a.ups = p.ups; a.stride = d->stride;
    a.OD = p.OD; a.OH = p.OH; a.OW = p.OW;
    a.pro_a = d->d_pro_a; a.pro_b = d->d_pro_b; a.gamma = d->d_gamma; a.beta = d->d_beta; a.act = d->act;
    a.bias = d->d_bias; a.cout = d->c_out; a.coutp = p.coutp;
    a.residual = d->d_residual; a.out = d->d_out;
    a.TX = p.TX; a.TY = p.TY; a.TZ = p.TZ; a.lTX = p.lTX; a.lTY = p.lTY;
    a.tiles_x = p.tiles_x; a.tiles_y = p.tiles_y; a.tiles_z = p.tiles_z; a.n_tiles = p.n_tiles;
    a.HX = p.HX; a.HY = p.HY; a.HZ = p.HZ; a.HYX = p.HYX; a.CS = p.CS; a.mHX = p.mHX; a.mHYX = p.mHYX;
    a.chunks_per_slice = p.chunks_per_slice; a.epi_lds = p.epi_lds;
    return a;
}

// called by pixie_conv3d_forward (conv3d_mfma.hip) when the descriptor carries f16x2-packed weights
int conv3d_f16x3_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st) {
    PX_REQUIRE(p.refusal != CONV_BAD_STRIDE, "f16x3 conv: stride must be 1, or 2 for a 3^3 kernel");
    PX_REQUIRE(p.refusal != CONV_BAD_CHANNELS, "f16x3 conv: c_in must be a multiple of 16 (got %d+%d)", d->c0, d->c1);
    PX_REQUIRE(d->d_in_amax0 != nullptr || d->in_bound > 0.0f, "f16x3 conv: needs d_in_amax0 or a positive in_bound");
    PX_REQUIRE(d->c1 == 0 || d->d_in_amax0 == nullptr || d->d_in_amax1 != nullptr, "f16x3 conv: second input needs its own amax slot");
    PX_REQUIRE(p.refusal != CONV_BAD_SUBPIXEL, "f16x3 conv: sub-pixel weights need upsample = 1, ksize = 3, stride = 1 and no folded skip");
    // the staging addresses a chunk's 16 channel planes with a 32-bit byte offset (raw buffer loads)
    PX_REQUIRE((int64_t)d->in_d * d->in_h * d->in_w * 16 * (int64_t)sizeof(float) < (int64_t)1 << 32, "f16x3 conv: 16 channels of the input must span less than 4 GiB");
    Conv16Args a = conv16_args(d, p);
    a.w16 = reinterpret_cast<const uint4*>(d->d_w16);
    a.amax0 = d->d_in_amax0; a.amax1 = (d->c1 > 0) ? d->d_in_amax1 : nullptr; a.in_bound = d->in_bound;
    a.stats = d->d_out_stats; a.out_amax = d->d_out_amax;
    if (d->d_skip_w16) {
        PX_REQUIRE(p.skip_foldable, "f16x3 conv: this launch cannot fold a skip convolution (pixie_conv_skip_foldable)");
        PX_REQUIRE(d->d_skip_in0 && d->d_skip_amax0 && (d->skip_c1 == 0 || (d->d_skip_in1 && d->d_skip_amax1)), "f16x3 conv: folded skip needs its inputs and their amax slots");
        // the register-fed skip loop addresses a chunk's 16 channels with a 32-bit byte offset
        PX_REQUIRE((int64_t)d->in_d * d->in_h * d->in_w * 16 * (int64_t)sizeof(float) < (int64_t)1 << 32, "f16x3 conv: folded skip: 16 channels of the skip input must span less than 4 GiB");
        a.sk_in0 = d->d_skip_in0; a.sk_in1 = d->d_skip_in1; a.sk_c0 = d->skip_c0; a.sk_cin = d->skip_c0 + d->skip_c1;
        a.sk_w16 = reinterpret_cast<const uint4*>(d->d_skip_w16); a.sk_bias = d->d_skip_bias;
        a.sk_amax0 = d->d_skip_amax0; a.sk_amax1 = d->skip_c1 > 0 ? d->d_skip_amax1 : nullptr;
    }
    if (p.slices > 1) {
        a.partial = static_cast<float*>(d->d_workspace);
        a.stats = nullptr; a.out_amax = nullptr;   // the conv kernel writes raw slices; the reduce takes the statistics
    }
    PX_REQUIRE(p.refusal != CONV_BAD_LDS, "f16x3 conv: tile needs %zu B of LDS", p.lds_bytes);
    PX_REQUIRE(p.f16x3(), "f16x3 conv: bad sizes");
    const size_t pair_lds = conv_pair_lds(p, a.sk_w16 != nullptr);
    if (int rc = launch(pair_lds ? conv16_pair_kernel(p) : conv16_kernel(p, a.sk_w16 != nullptr, a.sk_c0), p, a, st, pair_lds,
                        pair_lds ? nullptr : conv16_group_kernel(p, a.sk_w16 != nullptr)))
        return rc;
    if (p.slices == 1) return 0;
    const long osp = (long)a.OD * a.OH * a.OW, n_elems = (long)a.cout * osp;
    if (d->d_out_stats) {
        const dim3 rgrid((unsigned)reduce_segments(osp), (unsigned)a.cout);
        double* rstats = reinterpret_cast<double*>(d->d_out_stats);
        PX_REQUIRE((reinterpret_cast<size_t>(rstats) & 7) == 0, "f16x3 conv: d_out_stats of a split-K launch must be 8-byte aligned");
        const bool vec = osp % 4 == 0 && ((reinterpret_cast<size_t>(a.partial) | reinterpret_cast<size_t>(a.residual) | reinterpret_cast<size_t>(a.out)) & 15) == 0;
        if (vec) px_launch_grouped(splitk_reduce_stats_kernel<true>, splitk_reduce_stats_group_kernel<true>, rgrid, dim3(256), 0, st, a.partial, p.slices,
                                   n_elems, osp, a.bias, a.residual, a.out, rstats, d->d_out_amax);
        else px_launch_grouped(splitk_reduce_stats_kernel<false>, splitk_reduce_stats_group_kernel<false>, rgrid, dim3(256), 0, st, a.partial, p.slices,
                               n_elems, osp, a.bias, a.residual, a.out, rstats, d->d_out_amax);
    } else {
        px_launch(splitk_reduce_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, st, a.partial, p.slices, n_elems, osp,
                  a.bias, a.residual, a.out);
    }
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

// called by pixie_conv3d_forward (conv3d_mfma.hip) for exact-fp32 descriptors (d_w, no d_w16) that the plan sends through the
// tiled body (conv16_body.h) instead of the first-generation kernel
int conv3d_exact_forward(const pixie_conv_desc* d, const ConvPlan& p, hipStream_t st) {
    PX_REQUIRE(p.refusal != CONV_BAD_LDS, "exact conv: tile needs %zu B of LDS", p.lds_bytes);
    PX_REQUIRE(p.path == CONV_EXACT_TILED, "exact conv: bad sizes");
    Conv16Args a = conv16_args(d, p);
    a.wf = d->d_w;
    a.in_bound = 1.0f;
    return launch(conv16_kernel(p), p, a, st);
}

}  // namespace pixie

using namespace pixie;

static ConvPlan plan_of(const pixie_conv_desc* d) { return d ? conv_plan(conv_shape_of(d)) : ConvPlan{}; }
static StatParts stat_parts(const ConvPlan& p, const void* stats) { return StatParts{stats, p.stats.n, p.stats.cstride, p.stats.tstride, p.stats.f64}; }

// number of floats of the epilogue statistics buffer for this descriptor (0 if the layer does not take the f16x3 path)
extern "C" int64_t pixie_conv_stats_floats(const pixie_conv_desc* d) { return plan_of(d).stats_floats; }

// bytes of d_workspace this layer can use for split-K (0: it would not split).  Decided on the shape alone.
extern "C" int64_t pixie_conv_workspace_bytes(const pixie_conv_desc* d) {
    if (!d) return 0;
    ConvShape s = conv_shape_of(d);
    s.workspace = true;   // "a workspace would be available"
    return conv_plan(s).workspace_bytes;
}

// which kernel instantiation pixie_conv3d_forward picks for this descriptor: variant = ksize * 100 + MB * 10 + NB of
// conv3d_f16x3_kernel<ksize, MB, NB>, slices = its split-K factor; 0 = the exact-fp32 kernel.  (Lets a profiler group
// its own per-launch timings the way rocprofv3 groups them: by kernel name.)
#ifdef PIXIE_DIAG
extern "C" int pixie_conv_kernel_variant(const pixie_conv_desc* d, int* slices_out) {
    if (!d) {   // the launcher-form switch: *slices_out = 1 keeps the 4-wave kernels, 0 gives the choice back to the plan
        const int before = g_conv_keep_four_wave;
        if (slices_out && (*slices_out == 0 || *slices_out == 1)) g_conv_keep_four_wave = *slices_out;
        return before;
    }
    const ConvPlan p = plan_of(d);
    if (slices_out) *slices_out = p.f16x3() ? p.slices : 1;
    return conv_variant_number(p);
}

// the tiling pixie_conv3d_forward launches this descriptor with: out = TX, TY, TZ, tiles_x, tiles_y, tiles_z, epi_lds, slices,
// MB, NB.  With d_w16 the f16x3 launch (sub-pixel: the tile lies over the STORED voxels, each tile is four workgroups);
// without, the exact-fp32 launch of the same body.  Returns 1 (and leaves out alone) for descriptors that take neither.
extern "C" int pixie_conv_tile_geometry(const pixie_conv_desc* d, int32_t out[10]) {
    const ConvPlan p = plan_of(d);
    if (!out && d) return (int)conv_pair_lds(p, d->d_skip_w16 != nullptr);   // the launcher's form for this descriptor, as it is switched now
    return out && conv_tile_geometry(p, out) ? 0 : 1;
}

// where this descriptor's launch leaves its partial statistics, as pixie_stats_finalize / pixie_stats_norm_finalize will read them:
// out = partials per channel, cstride, tstride (in (sum, sum of squares) pairs), 1 = fp64 reduce segments /
// 0 = fp32 tile partials, voxels per reduce segment (0 for tile partials), c_out padded.  Returns 1 off the f16x3 path.
extern "C" int pixie_conv_stats_layout(const pixie_conv_desc* d, int64_t out[6]) {
    const ConvPlan p = plan_of(d);
    return out && conv_stats_layout(p, out) ? 0 : 1;
}
#endif

extern "C" int pixie_conv_skip_foldable(const pixie_conv_desc* d) { return plan_of(d).skip_foldable ? 1 : 0; }

extern "C" int pixie_stats_finalize(const float* d_stats, const pixie_conv_desc* d, double* d_sums, void* stream) {
    PX_REQUIRE(d_stats && d && d_sums, "pixie_stats_finalize: null argument");
    // the tile (or segment) count comes from the plan conv3d_f16x3_forward launched with
    px_launch(stats_finalize_kernel, dim3((unsigned)d->c_out), dim3(256), 0, as_stream(stream), stat_parts(plan_of(d), d_stats), d_sums);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_stats_norm_finalize(const float* d_stats0, const pixie_conv_desc* desc0, double* d_sums0, const float* d_stats1,
                                         const pixie_conv_desc* desc1, double* d_sums1, int c1, int64_t spatial, int mode, int groups,
                                         double eps, const float* d_weight, const float* d_bias, float* d_a, float* d_b, void* stream) {
    PX_REQUIRE(desc0 && d_sums0 && d_a && d_b && spatial > 0 && c1 >= 0, "pixie_stats_norm_finalize: bad arguments");
    PX_REQUIRE(c1 == 0 || d_sums1, "pixie_stats_norm_finalize: a second part needs d_sums1");
    PX_REQUIRE(!d_stats1 || desc1, "pixie_stats_norm_finalize: d_stats1 needs its descriptor");
    const int c0 = desc0->c_out, channels = c0 + c1;
    PX_REQUIRE(!d_stats1 || desc1->c_out == c1, "pixie_stats_norm_finalize: desc1 has %d output channels, c1 is %d", desc1 ? desc1->c_out : 0, c1);
    PX_REQUIRE(mode == 0 || (mode == 1 && groups > 0 && channels % groups == 0), "pixie_stats_norm_finalize: bad mode/groups");
    const StatParts none{nullptr, 0, 0, 0, 0};
    const StatParts p0 = d_stats0 ? stat_parts(plan_of(desc0), d_stats0) : none;
    const StatParts p1 = d_stats1 ? stat_parts(plan_of(desc1), d_stats1) : none;
    px_launch_grouped(stats_norm_finalize_kernel, stats_norm_finalize_group_kernel, dim3((unsigned)(mode == 0 ? channels : groups)), dim3(256), 0,
                      as_stream(stream), p0, d_sums0, c0, p1, d_sums1, channels, (double)spatial, mode, groups, eps, d_weight, d_bias, d_a, d_b);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t pixie_conv_packed16_bytes(int c_out, int c_in, int ksize) {
    if (c_out <= 0 || c_in <= 0 || c_in % 8 != 0 || (ksize != 1 && ksize != 3)) return 0;
    const int64_t taps = (int64_t)ksize * ksize * ksize;
    return ((int64_t)kW16HeaderU4 + 2 * taps * (c_in / 8) * pixie_conv_cout_padded(c_out)) * (int64_t)sizeof(uint4);
}

extern "C" int pixie_tensor_amax(const float* d_x, int64_t count, uint32_t* d_slot, void* stream) {
    PX_REQUIRE(d_x && d_slot && count > 0, "pixie_tensor_amax: bad arguments");
    const int blocks = (int)std::min<int64_t>(2048, (count + 1023) / 1024);
    hipLaunchKernelGGL(amax_kernel, dim3(blocks), dim3(256), 0, as_stream(stream), d_x, (long)count, d_slot);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int pixie_conv_pack_weights_f16x2(const float* d_w, void* d_packed, int c_out, int c_in, int ksize, void* stream) {
    PX_REQUIRE(d_w && d_packed && c_out > 0 && c_in > 0 && c_in % 8 == 0 && (ksize == 1 || ksize == 3),
               "pixie_conv_pack_weights_f16x2: bad arguments (c_in must be a multiple of 8)");
    hipStream_t st = as_stream(stream);
    const int taps = ksize * ksize * ksize;
    const int coutp = pixie_conv_cout_padded(c_out);
    // the |w|max slot lives in the header's last word until the pack kernel overwrites the header
    unsigned* slot = reinterpret_cast<unsigned*>(d_packed) + 15;
    PX_CHECK_HIP(hipMemsetAsync(d_packed, 0, kW16HeaderU4 * sizeof(uint4), st));
    if (pixie_tensor_amax(d_w, (int64_t)c_out * c_in * taps, slot, stream)) return 1;
    const long total = (long)taps * (c_in / 8) * coutp;
    hipLaunchKernelGGL(pack_weights_f16x2_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, d_w, reinterpret_cast<uint4*>(d_packed), c_out,
                       c_in, taps, coutp, slot);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

extern "C" int64_t pixie_conv_subpixel_bytes(int c_out, int c_in) {
    if (c_out <= 0 || c_in <= 0 || c_in % 16 != 0) return 0;
    return ((int64_t)kW16HeaderU4 + 2 * 64 * (int64_t)(c_in / 8) * pixie_conv_cout_padded(c_out)) * (int64_t)sizeof(uint4);
}

extern "C" int pixie_conv_pack_weights_subpixel(const float* d_w, void* d_packed, int c_out, int c_in, void* stream) {
    PX_REQUIRE(d_w && d_packed && c_out > 0 && c_in > 0 && c_in % 16 == 0,
               "pixie_conv_pack_weights_subpixel: bad arguments (c_in must be a multiple of 16)");
    hipStream_t st = as_stream(stream);
    const int coutp = pixie_conv_cout_padded(c_out);
    // as in pixie_conv_pack_weights_f16x2: the |w|max slot lives in the header's last word until the header is written
    unsigned* slot = reinterpret_cast<unsigned*>(d_packed) + 15;
    PX_CHECK_HIP(hipMemsetAsync(d_packed, 0, kW16HeaderU4 * sizeof(uint4), st));
    const long pairs = (long)c_out * c_in;
    hipLaunchKernelGGL(subpixel_amax_kernel, dim3(cdiv(pairs, 256)), dim3(256), 0, st, d_w, pairs, slot);
    PX_CHECK_HIP(hipGetLastError());
    const long total = 64L * (c_in / 8) * coutp;
    hipLaunchKernelGGL(pack_weights_subpixel_kernel, dim3(cdiv(total, 256)), dim3(256), 0, st, d_w, reinterpret_cast<uint4*>(d_packed), c_out,
                       c_in, coutp, slot);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}
