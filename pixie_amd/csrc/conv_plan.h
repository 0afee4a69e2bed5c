// pixie_amd/csrc/conv_plan.h -- the launch plan of one convolution: WHAT pixie_conv3d_forward launches for a descriptor.
//
// conv_plan() is a pure host function of the descriptor's shape fields and of flags that say which optional operands are given.
// The launchers copy its geometry into the kernel arguments; every size query and diagnostic of include/pixie_hip.h reads the same
// plan, and so does the U-Net executor (unet_exec.hip), for its dry run and its real pass alike.  A new tile rule or kernel variant
// changes conv_plan() and the one variant table, both below.
// Pure and self-contained: no HIP header, no pointer looked at, no environment read (conv_shape_of() and conv_exact_v1() in
// conv3d_f16x3.hip turn a descriptor and the environment into a ConvShape).  g++ compiles this header alone into a sanitized
// program for tests/test_conv_plan_host.py, which holds it to tests/golden/conv_plan_table.json row by row.
#pragma once
#include <algorithm>
#include <cstddef>
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
    size_t lds_bytes = 0;
    unsigned grid_x = 1, grid_y = 1, grid_z = 1;   // the 4-wave launch: tiles, blocks of MB * 32 output channels, split-K slices
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
// c_out rounded up to whole 32-row MFMA blocks: what pixie_conv_cout_padded answers
inline int conv_cout_padded(int c_out) { return (c_out + 31) / 32 * 32; }

// split-K launches: voxels of one channel a workgroup of splitk_reduce_stats_kernel (conv_stat_kernels.h) owns, and the segments
// per channel = partial statistics per channel
constexpr int kReduceSeg = 4096;
inline int reduce_segments(long osp) { return (int)((osp + kReduceSeg - 1) / kReduceSeg); }

// the output dims of a convolution: padding ksize / 2, nearest x2 upsampling first, cropped to out_* where given
inline void conv_output_dims(const ConvShape& s, int& od, int& oh, int& ow) {
    const int pad = s.ksize == 3 ? 1 : 0;
    od = ((s.in_d << s.upsample) + 2 * pad - s.ksize) / s.stride + 1;
    oh = ((s.in_h << s.upsample) + 2 * pad - s.ksize) / s.stride + 1;
    ow = ((s.in_w << s.upsample) + 2 * pad - s.ksize) / s.stride + 1;
    if (s.out_d > 0) od = std::min(od, s.out_d);   // odd-grid crop (diffusion_network.py:925-930)
    if (s.out_h > 0) oh = std::min(oh, s.out_h);
    if (s.out_w > 0) ow = std::min(ow, s.out_w);
}

// Path, kernel entry, split factor, tile and buffer sizes of one launch.  A refused plan (path CONV_NONE) says why and keeps what
// was decided up to there (output dims, LDS request) for the caller's message; its buffer sizes are still 0.
inline ConvPlan conv_plan(const ConvShape& s) {
    ConvPlan p;
    auto refuse = [&p](ConvRefusal why) { p.path = CONV_NONE; p.refusal = why; return p; };
    if ((s.ksize != 1 && s.ksize != 3) || (s.stride != 1 && s.stride != 2) || (s.upsample != 0 && s.upsample != 1) || s.c0 <= 0 || s.c1 < 0 ||
        s.c_out <= 0 || s.in_d <= 0 || s.in_h <= 0 || s.in_w <= 0)
        return refuse(CONV_BAD_SHAPE);
    conv_output_dims(s, p.OD, p.OH, p.OW);
    p.KS = s.ksize; p.coutp = conv_cout_padded(s.c_out);
    p.ups = s.upsample; p.LD = s.in_d << p.ups; p.LH = s.in_h << p.ups; p.LW = s.in_w << p.ups;
    // which path: the tiled body takes 16-channel chunks, and stride 2 only under a 3^3 kernel without upsampling (the Downsample
    // convs); its f16x3 form reads the first input in groups of 8 channels.  Exact-fp32 descriptors that do not fit keep the
    // first-generation kernel of conv3d_mfma.hip (odd channel counts, tiny test networks); f16x3 ones are refused.
    const int cin = s.c0 + s.c1;
    const bool stride_ok = s.stride == 1 || (s.ksize == 3 && !s.upsample), chunks_ok = cin % 16 == 0;
    if (!s.w16) {
        if (!stride_ok || !chunks_ok || s.exact_v1) { p.path = CONV_FIRST_GEN; return p; }
        p.path = CONV_EXACT_TILED;
    } else {
        if (!stride_ok) return refuse(CONV_BAD_STRIDE);
        if (!chunks_ok || s.c0 % 8 != 0) return refuse(CONV_BAD_CHANNELS);
        // (subpixel says how the weights were packed; the shape must allow it)
        if (s.subpixel && !(s.upsample == 1 && s.ksize == 3 && s.stride == 1 && !s.skip)) return refuse(CONV_BAD_SUBPIXEL);
        p.path = s.subpixel ? CONV_F16X3_SUBPIXEL : CONV_F16X3;
    }
    const bool sub = p.path == CONV_F16X3_SUBPIXEL;
    const int chunks = cin / 16;
    const int smax = (p.f16x3() && s.workspace) ? std::min(8, chunks / 2) : 1;   // no split-K on the exact path: small layers shrink the tile instead
    // a tile of at most `vox` voxels over an extent
    auto tile = [&p](int ED, int EH, int EW, int vox) {
        p.TX = pow2_le(EW, 32);
        p.TY = pow2_le(EH, std::max(1, std::min(4, vox / p.TX)));
        p.TZ = std::max(1, std::min(ED, vox / (p.TX * p.TY)));
        p.lTX = ilog2(p.TX); p.lTY = ilog2(p.TY);
        p.tiles_x = (EW + p.TX - 1) / p.TX; p.tiles_y = (EH + p.TY - 1) / p.TY; p.tiles_z = (ED + p.TZ - 1) / p.TZ;
        p.n_tiles = p.tiles_x * p.tiles_y * p.tiles_z;
    };
    if (sub) {
        // the tile lies over the STORED voxels that have an output: 4 waves x 64 voxels, each worth two x parities; one
        // workgroup per tile and (z, y) parity, the parity fastest: where the body's XCD remap applies and the tile count is a
        // multiple of 8 (every shape of the 128^3 network) the four parities of a tile run in one XCD and share their input in
        // its L2; otherwise they may straddle XCDs and meet in the MALL instead (performance only)
        p.ups = 0; p.LD = s.in_d; p.LH = s.in_h; p.LW = s.in_w;
        tile((p.OD + 1) / 2, (p.OH + 1) / 2, (p.OW + 1) / 2, 256);
        p.n_tiles *= 4;
        p.HX = p.TX + 2; p.HY = p.TY + 1; p.HZ = p.TZ + 1;
        p.MB = (p.coutp >= 64) ? 2 : 1; p.NB = 4;
        // too few workgroups for the chip: split the channel chunks (needs the caller's workspace)
        const long wgs = (long)p.n_tiles * ((p.coutp + p.MB * 32 - 1) / (p.MB * 32));
        while (p.slices * 2 <= smax && wgs * p.slices < 512) p.slices *= 2;
    } else {
        const long ovol = (long)p.OD * p.OH * p.OW;
        int MB = (p.coutp >= 64) ? 2 : 1;
        int NB = (s.stride == 2) ? 1 : 4;   // stride 2: the tile holds 8x the voxels it produces; only NB = 1 fits (112 KB, one workgroup per CU)
        auto n_wg = [&](int mb, int nb) {
            const long tiles = (ovol + 128L * nb - 1) / (128L * nb);
            return tiles * ((p.coutp + mb * 32 - 1) / (mb * 32));
        };
        // Split-K (needs the caller's workspace): when the output is too small to give every CU two workgroups, keep the
        // big MFMA-efficient tile and split the channel chunks over up to 8 slices instead of shrinking the tile; the
        // slices write partial outputs that splitk_reduce_kernel adds in a fixed order.
        int slices = 1;
        if (smax >= 2 && n_wg(MB, NB) < 512) {
            bool found = false;
            for (int nb = NB; nb >= 1 && !found; nb /= 2) {
                for (int sl = 1; sl <= smax; sl *= 2)
                    if (n_wg(MB, nb) * sl >= 512) { NB = nb; slices = sl; found = true; break; }
            }
            if (!found) { NB = 1; slices = 1; while (slices * 2 <= smax) slices *= 2; }
        } else {
            while (n_wg(MB, NB) < 512 && NB > 1) NB /= 2;
            if (n_wg(MB, NB) < 512 && MB > 1) MB = 1;
        }
        p.MB = MB; p.NB = NB; p.slices = slices;
        tile(p.OD, p.OH, p.OW, 128 * NB);
        p.HX = (p.TX - 1) * s.stride + s.ksize; p.HY = (p.TY - 1) * s.stride + s.ksize; p.HZ = (p.TZ - 1) * s.stride + s.ksize;
    }
    p.HYX = p.HY * p.HX; p.CS = p.HZ * p.HYX;
    p.mHX = magic_of(p.HX); p.mHYX = magic_of(p.HYX);
    if (p.slices > 1) p.chunks_per_slice = (chunks + p.slices - 1) / p.slices;
    p.lds_bytes = (size_t)4 * p.CS * 16;   // four 16-byte fp16 planes per halo voxel (exact: 16 fp32 planes)
    if (p.lds_bytes > 160 * 1024) return refuse(CONV_BAD_LDS);
    // LDS the transposing epilogue needs (4 waves x 32 rows x (NB*32 + 4) floats + the statistics partials), and whether the launch
    // gets it: unsplit launches only, as long as two workgroups still fit on a CU
    const size_t epi_bytes = ((size_t)4 * 32 * (p.NB * 32 + 4) + (size_t)4 * p.MB * 32 * 2) * sizeof(float);
    if (p.slices == 1 && epi_bytes <= 80 * 1024) { p.epi_lds = 1; p.lds_bytes = std::max(p.lds_bytes, epi_bytes); }
    p.grid_x = (unsigned)p.n_tiles; p.grid_y = (unsigned)((p.coutp + p.MB * 32 - 1) / (p.MB * 32)); p.grid_z = (unsigned)p.slices;
    if (!p.f16x3()) return p;
    // where the launch leaves its partial statistics (d_out_stats): per tile in fp32, or per reduce segment in fp64
    const long osp = (long)p.OD * p.OH * p.OW;
    if (p.slices > 1) {
        const int n = reduce_segments(osp);
        p.stats = ConvStatLayout{n, n, 1, 1};
        p.stats_floats = (int64_t)s.c_out * n * 2 * (int64_t)(sizeof(double) / sizeof(float));
        p.workspace_bytes = (int64_t)p.slices * s.c_out * osp * (int64_t)sizeof(float);
    } else {
        p.stats = ConvStatLayout{p.n_tiles, 1, p.coutp, 0};
        p.stats_floats = (int64_t)p.n_tiles * p.coutp * 2;
    }
    // the full-resolution 64 -> 64 layers: the <3,2,4> code under its own symbol
    p.fullres = !sub && p.slices == 1 && s.ksize == 3 && p.MB == 2 && p.NB == 4 && cin == 64 && s.c_out == 64 && s.stride == 1 && !s.upsample &&
                s.c1 == 0 && !s.skip && osp >= 128L * 128 * 128;
    const int scin = s.skip_c0 + s.skip_c1;
    p.skip_foldable = !sub && s.stride == 1 && !s.upsample && scin > 0 && scin % 16 == 0 && s.skip_c0 % 8 == 0 && p.slices == 1;
    return p;
}

// The pair form of a planned launch (conv3d_f16x3_pair_kernel): the same plan -- tile, MB, NB, variant number, statistics layout
// -- launched with 512 threads over (n_tiles, coutp / 128).  A pure function of the plan and of whether a folded skip rides
// along: the plain f16x3 path, MB = 2, an even number of 64-channel blocks, and two tile buffers (or the eight waves' transposing
// epilogue area and statistics partials) within the 160 KB of a CU, which excludes every stride-2 tile.  Unsplit NB = 4 launches
// only: those are the classes that cleared the 2 % bar against their 4-wave form (profiles/conv_pair_pricing.txt: the 128^3
// launches -9.8 % and -18.3 %; the split-K launches of the 32^3 and 16^3 levels -1.1 % .. +4.8 %, so they keep the 4-wave kernels,
// and no launch of the networks reaches NB < 4 unsplit with 128 channels).  Returns the launch's dynamic LDS bytes, 0 = the launch
// keeps the 4-wave kernel.  (The diagnostic build can switch the form off: conv_pair_lds() in conv3d_f16x3.hip asks its switch first.)
inline size_t conv_pair_lds_bytes(const ConvPlan& p, bool skip) {
    if (p.path != CONV_F16X3 || p.fullres || skip || p.MB != 2 || p.NB != 4 || p.slices != 1 || p.coutp % 128 != 0) return 0;
    const size_t tiles = (size_t)2 * 4 * p.CS * 16;
    const size_t red = (size_t)2 * 4 * p.MB * 32 * 2 * sizeof(float);
    const size_t epi = p.epi_lds ? (size_t)8 * 32 * (p.NB * 32 + 4) * sizeof(float) + red : red;
    const size_t lds = std::max(tiles, epi);
    return lds <= 160 * 1024 ? lds : 0;
}

// What the diagnostic queries of include/pixie_hip.h answer in the diagnostic build, as functions of the plan.  (The macro that selects that
// build is not named in this header: build.py compiles twice every source that, itself or through a header, mentions it.)
// pixie_conv_kernel_variant: ksize * 100 + MB * 10 + NB of conv3d_f16x3_kernel<ksize, MB, NB>; 8300 + MB * 10 + NB for
// conv3d_f16x3_subpixel_kernel<MB>; 9324 for conv3d_f16x3_c64_fullres_kernel; 0 off the f16x3 paths
inline int conv_variant_number(const ConvPlan& p) {
    if (!p.f16x3()) return 0;
    if (p.path == CONV_F16X3_SUBPIXEL) return 8300 + p.MB * 10 + p.NB;
    if (p.fullres) return 9324;
    return p.KS * 100 + p.MB * 10 + p.NB;
}
// pixie_conv_tile_geometry: TX, TY, TZ, tiles_x, tiles_y, tiles_z, epi_lds, slices, MB, NB; false (out left alone) off the tiled paths
inline bool conv_tile_geometry(const ConvPlan& p, int32_t out[10]) {
    if (!p.tiled()) return false;
    const int32_t v[10] = {p.TX, p.TY, p.TZ, p.tiles_x, p.tiles_y, p.tiles_z, p.epi_lds, p.slices, p.MB, p.NB};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return true;
}
// pixie_conv_stats_layout: partials per channel, cstride, tstride, 1 = fp64 reduce segments / 0 = fp32 tile partials, voxels per
// reduce segment (0 for tile partials), c_out padded; false (out left alone) off the f16x3 paths
inline bool conv_stats_layout(const ConvPlan& p, int64_t out[6]) {
    if (!p.f16x3()) return false;
    out[0] = p.stats.n; out[1] = p.stats.cstride; out[2] = p.stats.tstride; out[3] = p.stats.f64; out[4] = p.stats.f64 ? kReduceSeg : 0;
    out[5] = p.coutp;
    return true;
}

}  // namespace pixie
