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
//   A: weights are pre-split and pre-swizzled on the device (pack kernel below) into [tap][k-group][c_out] x 16 B
//      hi/lo planes; every wave reads its A fragments straight from L2 (two coalesced 512 B segments per load;
//      the whole 64->64 3^3 layer is 442 KB), so LDS holds activations only and two workgroups fit per CU.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <map>
#include <string>
#include <type_traits>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "conv_plan.h"

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
    float* stats; unsigned* out_amax;   // epilogue statistics (see the epilogue), or null
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

// One tiled body, two arithmetic variants.  256 threads = 4 waves; two workgroups share a CU (their staging and MFMA phases
// overlap by occupancy).  Rejected and removed after measurement (profiles/README.md r1w): a wave-specialised
// 512-thread variant (4 MFMA + 4 staging waves: 1.95 vs 1.54 ms) and a software-pipelined one-workgroup-per-CU variant
// (1.74-1.89 vs 1.59 ms); the timing-study switches that used to live in the tap loop are gone with them.
// EX ("exact"): the same tiling, staging, prologue and epilogue with fp32 operands on v_mfma_f32_32x32x2_f32 -- every product
// and every accumulation in fp32, as the reference's cuDNN/PyTorch fp32 convolution computes them (conv_precision = "f32").
// The LDS tile holds the 16 channels of a chunk as fp32 planes [channel][voxel] (the same 64 bytes per voxel as the four
// fp16 planes), a lane's B operand is one conflict-free ds_read_b32, its A operand one coalesced 4-byte load from the
// [tap][c_in][c_out] weight array (L2-resident: 442 KB for the 64 -> 64 layer), fetched one tap ahead.
// (Round 5 tried taking the dx = 1, 2 B fragments of a row from the neighbouring lane with v_mov_b32_dpp wave_shl:1 instead of two more
// LDS reads: 1.45 vs 1.30 ms on the dominant layer, 1.97 vs 1.78 J per launch -- profiles/r5c_conv_dppb_rejected.txt.)
// SP ("sub-pixel"): a 3^3 convolution behind a nearest x2 upsampling, computed over the STORED tensor.  Output voxel 2i + p reads
// floor((2i + p + d) / 2) for d = -1, 0, 1: i-1, i, i for p = 0 and i, i, i+1 for p = 1, so per axis two effective taps with
// pre-summed weights (pack_weights_subpixel_kernel) and per output parity a 2x2x2 convolution: 8 taps instead of 27.  A
// workgroup takes one (z, y) parity (tile index & 3) and BOTH x parities of a tile of 4 x 64 stored voxels: accumulator
// block nb = 2 px + s holds x parity px of the wave's stored-voxel block s, so the transposing epilogue writes whole output
// rows.  The tile is staged without the x2 replication with a halo of one voxel on the side the parity reads
// (x: both sides), i.e. (TX + 2)(TY + 1)(TZ + 1) slots; A.ups is 0 and A.L* are the stored dims on this path.
// PAIR ("pair form", launches with an even number of 64-channel blocks): 512 threads = two quartets of 4 waves over ONE tile;
// quartet q computes the c_out block 2 blockIdx.y + q and each of its waves is the 4-wave form's wave (same voxels, same A rows,
// same order of chunks, taps and terms: the results are the 4-wave form's bit for bit).  The tile is staged once for both
// quartets into two LDS buffers: chunk 0 by all 512 threads, then per chunk k quartet 0 stages its half of chunk k + 1's slots
// and multiplies chunk k, quartet 1 multiplies first and stages afterwards, one barrier per chunk.  Waves w and w + 4 share a
// SIMD, so each SIMD has one wave in the tap loop while the other stages.
template <int KS, int MB, int NB, bool EX = false, bool SP = false, int SK = 0, bool PAIR = false>
__device__ __forceinline__ void conv3d_f16x3_body(const Conv16Args& A) {
    static_assert(!PAIR || (MB == 2 && !EX && !SP && SK == 0), "pair form: the plain f16x3 body with 64 c_out per quartet");
    static_assert(!SP || (KS == 3 && NB == 4 && !EX), "sub-pixel path: 3^3, two x parities x two voxel blocks per wave");
    static_assert(SK == 0 || (!EX && !SP), "folded skip (SK: 1 register-fed, 2 staged through LDS): f16x3, no sub-pixel form");
    extern __shared__ uint4 smem16[];
    constexpr int PAD = (KS == 3) ? 1 : 0;
    constexpr int NW = 4, NT = 64 * NW;     // (an 8-wave, one-workgroup-per-CU tile was measured in round 4: 1.350 vs 1.323 ms, profiles/r4k_conv_eight_wave_tile_rejected.txt)
    const int bufsz = 4 * A.CS;            // one buffer: hi[2][CS], lo[2][CS]

    const int tid = threadIdx.x;
    const int lane = tid & 63;
    const int quartet = PAIR ? __builtin_amdgcn_readfirstlane(tid >> 8) : 0;   // wave-uniform
    const int wave = PAIR ? (tid >> 6) & 3 : tid >> 6;                           // within the quartet
    const int qtid = PAIR ? tid & 255 : tid;
    const int kh = lane >> 5;
    const int l31 = lane & 31;

    // XCD-aware tile order: consecutive workgroups go to different XCDs (b % 8), so give each XCD a contiguous
    // run of tiles -- neighbouring tiles then share their halo planes in that XCD's L2.
    int t = blockIdx.x;
    {
        const int per = (A.n_tiles + 7) >> 3;
        const int cand = (t & 7) * per + (t >> 3);
        // exact only when n_tiles is a multiple of 8; otherwise keep the identity order
        if ((A.n_tiles & 7) == 0) t = cand;
    }
    int par = 0;                                  // SP: (z, y) output parity of this workgroup
    if constexpr (SP) { par = t & 3; t >>= 2; }
    const int py = par & 1, pz = par >> 1;
    const int tx = t % A.tiles_x; t /= A.tiles_x;
    const int ty = t % A.tiles_y;
    const int tz = t / A.tiles_y;
    const int ox0 = tx * A.TX, oy0 = ty * A.TY, oz0 = tz * A.TZ;   // SP: in stored voxels
    const int cout0 = (PAIR ? 2 * (int)blockIdx.y + quartet : (int)blockIdx.y) * (MB * 32);
    const int lx0 = SP ? ox0 - 1 : ox0 * A.stride - PAD;
    const int ly0 = SP ? oy0 - 1 + py : oy0 * A.stride - PAD;
    const int lz0 = SP ? oz0 - 1 + pz : oz0 * A.stride - PAD;
    const size_t ISP = (size_t)A.ID * A.IH * A.IW;
    const size_t OSP = (size_t)A.OD * A.OH * A.OW;

    int voff[NB];
    int ovox[NB];
    bool valid[NB];
#pragma unroll
    for (int nb = 0; nb < NB; ++nb) {
        if constexpr (SP) {
            const int px = nb >> 1;
            const int j = (wave * 2 + (nb & 1)) * 32 + l31;
            int x = j & (A.TX - 1);
            int y = (j >> A.lTX) & (A.TY - 1);
            int z = j >> (A.lTX + A.lTY);
            const int gx = 2 * (ox0 + x) + px, gy = 2 * (oy0 + y) + py, gz = 2 * (oz0 + z) + pz;
            const bool v = (z < A.TZ) && (gx < A.OW) && (gy < A.OH) && (gz < A.OD);
            if (!v) { x = 0; y = 0; z = 0; }
            voff[nb] = (z * A.HY + y) * A.HX + x + px + kh * A.CS;
            ovox[nb] = v ? (gz * A.OH + gy) * A.OW + gx : 0;
            valid[nb] = v;
            continue;
        }
        const int j = (wave * NB + nb) * 32 + l31;
        int x = j & (A.TX - 1);
        int y = (j >> A.lTX) & (A.TY - 1);
        int z = j >> (A.lTX + A.lTY);
        const bool v = (z < A.TZ) && (ox0 + x < A.OW) && (oy0 + y < A.OH) && (oz0 + z < A.OD);
        if (!v) { x = 0; y = 0; z = 0; }
        voff[nb] = ((z * A.HY + y) * A.HX + x) * A.stride + kh * A.CS;
        ovox[nb] = ((oz0 + z) * A.OH + (oy0 + y)) * A.OW + ox0 + x;
        valid[nb] = v;
    }

    // input scale
    float bound = A.in_bound;
    if (A.amax0) {
        bound = __uint_as_float(*A.amax0);
        if (A.amax1) bound = fmaxf(bound, __uint_as_float(*A.amax1));
    }
    const int ex = EX ? 0 : scale_exponent(bound);
    const float sx = pow2i(ex);

    f32x16 acc[MB][NB];
#pragma unroll
    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
        for (int nb = 0; nb < NB; ++nb)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[mb][nb][r] = 0.0f;

    const int KG = A.cin >> 3;                              // 8-channel groups
    const size_t tap_stride = (size_t)KG * A.coutp;         // uint4 units
    const size_t plane = (size_t)(SP ? 64 : KS * KS * KS) * tap_stride;   // SP: [parity (pz, py, px)][tap (ez, ey, ex)]
    const uint4* wHi = A.w16 + kW16HeaderU4 + (size_t)kh * A.coutp + cout0 + l31 + (size_t)(par * 16) * tap_stride;
    const uint4* wLo = wHi + plane;
    const float* wF = A.wf + (size_t)kh * A.coutp + cout0 + l31;     // EX: channel (2 kp + kh) of the pair, row l31 of block mb

    constexpr int TAPS = KS * KS * KS;
    // ---- stage the 16-channel chunk starting at c_base into `buf`: one voxel x 16 channels per item.  A thread owns the items
    // k = 0 .. n - 1 at slots s0 + stid + nthr k of the slot range [s0, s1), n = ceil((s1 - s0) / nthr) (uniform over the staging
    // threads; the 4-wave form stages [0, CS) with all its threads: 5 at the 34 x 6 x 6 tile), and walks them as a
    // rotating pipeline over two register sets: the 16 + 2 loads of item k + 1 are issued -- behind its geometry, which is computed
    // under the flight of item k -- before item k is converted and written, so a chunk exposes ONE global-memory round trip and
    // every later conversion waits with a counted vmcnt while the younger item is in flight.  The loop is unrolled by two so that
    // neither set is ever copied, and the last one or two items are peeled: a load behind a branch would make the wait in front
    // of the older item a full one.  (Before: passes of two items per thread, each pass load -> wait -> convert -> store, three
    // exposed round trips at that tile and 1536 item slots for 1224; profiles/conv_staging_pricing.txt.)
    // Everything uniform is kept out of the per-element code: the channel base pointers are scalar,
    // the 32 per-channel prologue constants are fetched with ONE vector load per wave and broadcast into SGPRs with
    // v_readlane, out-of-range voxels load element 0 (masked after the activation) so the 16 + 2 loads of an item
    // issue back to back without exec-mask branches, and the (has-prologue, activation) switch selects one of six
    // straight-line pipelines.  (The first version left those decisions to per-element code; the compiler
    // turned the constants into dependent vector loads with s_waitcnt vmcnt(0) -- 16 of the 27 us a chunk took.)
    auto stage_chunk = [&](int c_base, uint4* buf, int stid, int nthr, int s0, int s1) {
        uint4* bHi = buf;
        uint4* bLo = buf + 2 * A.CS;
        float pa[16], pb[16];
        {
            float pv = 0.0f;
            if (A.pro_a) pv = (lane & 16) ? A.pro_b[c_base + (lane & 15)] : A.pro_a[c_base + (lane & 15)];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                pa[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pv), j));
                pb[j] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pv), 16 + j));
            }
        }
        const bool has_aff = A.gamma != nullptr;
        using T = std::true_type; using F = std::false_type;
        if constexpr (EX) {
            // the exact-fp32 body keeps the two-items-per-pass loop: the pipeline below costs it registers (<3,2,4>: 243 -> 256
            // VGPRs and spills, <3,2,2>: occupancy 3 -> 2; profiles/conv_staging_kernel_resources_after.txt has the f16x3 side)
            float* bF = reinterpret_cast<float*>(buf);
            for (int v0 = stid; v0 < A.CS; v0 += 2 * nthr) {
                float val[2][16];
                float gm[2], bt[2];
                int sidx[2];
                bool ok[2];
#pragma unroll
                for (int u = 0; u < 2; ++u) {
                    const int vox = v0 + u * nthr;
                    int rem = vox;
                    const int hz = fast_div16(rem, A.HYX, A.mHYX);
                    rem -= hz * A.HYX;
                    const int hy = fast_div16(rem, A.HX, A.mHX);
                    const int hx = rem - hy * A.HX;
                    const int lz = lz0 + hz, ly = ly0 + hy, lx = lx0 + hx;
                    ok[u] = vox < A.CS && (unsigned)lz < (unsigned)A.LD && (unsigned)ly < (unsigned)A.LH && (unsigned)lx < (unsigned)A.LW;
                    sidx[u] = ok[u] ? ((lz >> A.ups) * A.IH + (ly >> A.ups)) * A.IW + (lx >> A.ups) : 0;
                }
#pragma unroll
                for (int u = 0; u < 2; ++u) {
#pragma unroll
                    for (int j = 0; j < 16; ++j) {
                        const int cg = c_base + j;
                        const float* src = (cg < A.c0) ? (A.in0 + (size_t)cg * ISP) : (A.in1 + (size_t)(cg - A.c0) * ISP);
                        val[u][j] = src[sidx[u]];
                    }
                    gm[u] = 1.0f; bt[u] = 0.0f;
                    if (has_aff) { gm[u] = A.gamma[sidx[u]]; bt[u] = A.beta[sidx[u]]; }
                }
                auto convert = [&](auto has_pro, auto act_c) {
#pragma unroll
                    for (int u = 0; u < 2; ++u) {
                        const int vox = v0 + u * nthr;
#pragma unroll
                        for (int j = 0; j < 16; ++j) {
                            float t = val[u][j];
                            if (decltype(has_pro)::value) t = t * pa[j] + pb[j];
                            t = t * gm[u] + bt[u];
                            const float sc = ok[u] ? act16(t, decltype(act_c)::value) : 0.0f;   // zero padding AFTER the activation
                            if (vox < A.CS) bF[j * A.CS + vox] = sc;
                        }
                    }
                };
                if (A.pro_a) {
                    if (A.act == 1) convert(T{}, std::integral_constant<int, 1>{});
                    else if (A.act == 2) convert(T{}, std::integral_constant<int, 2>{});
                    else convert(T{}, std::integral_constant<int, 0>{});
                } else {
                    if (A.act == 1) convert(F{}, std::integral_constant<int, 1>{});
                    else if (A.act == 2) convert(F{}, std::integral_constant<int, 2>{});
                    else convert(F{}, std::integral_constant<int, 0>{});
                }
            }
            return;
        }
        const int n_items = (s1 - s0 + nthr - 1) / nthr;
        // The LayerNorm affine is fetched FIRST and without a branch (no affine: any readable element, replaced by 1 and 0 in the
        // conversion): every element's conversion needs it, and a load that may or may not have been issued behind the older
        // item's would turn that item's counted wait into one that also drains the head of the younger.  Without an affine the two
        // loads read in0[sidx] (in0 is never null and holds c0 >= 1 channels of ISP elements, so the index is in range) and are
        // discarded: 18 loads per item where the old loop issued 16.  That cost is not priced on its own; the launches without an
        // affine (sub-pixel up-convs, 1x1x1, stride 2) are in profiles/conv_staging_{before,after}_kernel_stats_by_geometry.csv.
        const float* gsrc = has_aff ? A.gamma : A.in0;
        const float* bsrc = has_aff ? A.beta : A.in0;
        // Addresses, as in the register-fed skip below: raw buffer loads over the chunk's first channel plane, the plane as the scalar
        // offset, the slot's voxel as the 32-bit vector offset (the launcher checks that 16 planes span less than 4 GiB).  With 64-bit
        // pointers an item pays 16 v_lshl_add_u64 and the 16 plane bases take 32 SGPRs.  Only where that lowers the registers: the
        // 3^3 instantiations with 64 c_out per wave and two or four voxel blocks (<3,2,4>, c64_fullres, <3,2,2>: 2 - 3 VGPRs fewer,
        // 3 - 5 % per launch); every other instantiation needs 6 - 17 VGPRs MORE with them (the descriptors and plane offsets
        // overflow the scalar file into VGPR lanes) and <1,2,2>, <1,2,1>, <1,1,2> lose a wave of occupancy, so those keep the
        // pointers.  A chunk that holds channels of both input tensors (c0 % 16 != 0; no layer of the networks)
        // keeps the pointers too, in a plain loop of its own (pipeline): picking the resource per channel costs 11 - 15 VGPRs
        // everywhere, and a branch around the loads spills at <3,2,4>.
        constexpr bool BUF = KS == 3 && MB == 2 && NB >= 2 && !SP;
        const unsigned chb = 4u * (unsigned)ISP;     // bytes per channel plane
        const int j1 = A.c0 - c_base;                // the chunk's first channel that lies in in1 (<= 0: all of them, >= 16: none)
        const bool straddle = j1 > 0 && j1 < 16;
        const float* cbase = (j1 > 0) ? A.in0 + (size_t)c_base * ISP : A.in1 + (size_t)(c_base - A.c0) * ISP;
        const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(cbase), 0, -1, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsg = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(gsrc), 0, -1, 0x00020000);
        const __amdgpu_buffer_rsrc_t rsb = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(bsrc), 0, -1, 0x00020000);
        struct Item { float val[16]; float gm, bt; bool ok; };
        // geometry of the item at slot `vox`: whether it lies inside the input, and its element in a channel plane (outside: element 0)
        auto slot = [&](int vox, bool& ok) {
            int rem = vox;
            const int hz = fast_div16(rem, A.HYX, A.mHYX);
            rem -= hz * A.HYX;
            const int hy = fast_div16(rem, A.HX, A.mHX);
            const int hx = rem - hy * A.HX;
            const int lz = lz0 + hz, ly = ly0 + hy, lx = lx0 + hx;
            ok = vox < s1 && (unsigned)lz < (unsigned)A.LD && (unsigned)ly < (unsigned)A.LH && (unsigned)lx < (unsigned)A.LW;
            return ok ? ((lz >> A.ups) * A.IH + (ly >> A.ups)) * A.IW + (lx >> A.ups) : 0;
        };
        auto load_with_pointers = [&](Item& it, int sidx) {
            it.gm = gsrc[sidx]; it.bt = bsrc[sidx];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                const int cg = c_base + j;
                const float* src = (cg < A.c0) ? (A.in0 + (size_t)cg * ISP) : (A.in1 + (size_t)(cg - A.c0) * ISP);
                it.val[j] = src[sidx];
            }
        };
        // the item's geometry, then its loads; nothing here waits for memory
        auto fetch = [&](Item& it, int vox) {
            const int sidx = slot(vox, it.ok);
            if constexpr (BUF) {
                const int voff = 4 * sidx;   // bytes into a plane
                it.gm = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsg, voff, 0, 0));
                it.bt = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsb, voff, 0, 0));
#pragma unroll
                for (int j = 0; j < 16; ++j)
                    it.val[j] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rs, voff, (int)((unsigned)j * chb), 0));
            } else {
                load_with_pointers(it, sidx);
            }
            // keep these loads above the conversion of the item before: left alone, the scheduler sinks them to their first use
            __builtin_amdgcn_sched_barrier(0);
        };
        auto convert = [&](const Item& it, int vox, auto has_pro, auto act_c) {
            const float gm = has_aff ? it.gm : 1.0f, bt = has_aff ? it.bt : 0.0f;
            // Straight-line for every slot, the masked ones included (they hold element 0 of each plane): a select in front of the
            // activation left SiLU one exec-masked block per element (s_and_saveexec, the full division, a wait of its own) and
            // kept the hi / lo split from being packed.
            f16x8 vh[2], vl[2];
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                float t = it.val[j];
                if (decltype(has_pro)::value) t = t * pa[j] + pb[j];
                t = t * gm + bt;
                const float sc = act16_staged(t, decltype(act_c)::value) * sx;
                const _Float16 h = (_Float16)sc;
                vh[j >> 3][j & 7] = h;
                vl[j >> 3][j & 7] = (_Float16)(sc - (float)h);
            }
            // zero padding AFTER the activation: a select on the 8 + 8 packed words, whatever the masked slot computed (NaN, inf)
            uint4 w[4] = {__builtin_bit_cast(uint4, vh[0]), __builtin_bit_cast(uint4, vh[1]), __builtin_bit_cast(uint4, vl[0]),
                          __builtin_bit_cast(uint4, vl[1])};
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                w[q].x = it.ok ? w[q].x : 0u; w[q].y = it.ok ? w[q].y : 0u;
                w[q].z = it.ok ? w[q].z : 0u; w[q].w = it.ok ? w[q].w : 0u;
            }
            if (vox < s1) {
                bHi[vox] = w[0];
                bHi[A.CS + vox] = w[1];
                bLo[vox] = w[2];
                bLo[A.CS + vox] = w[3];
            }
            __builtin_amdgcn_sched_barrier(0);   // the next fetch reuses this set: it stays below
        };
        auto pipeline = [&](auto has_pro, auto act_c) {
            Item a, b;
            int vox = s0 + stid;         // slot of the item in `a`; the one in `b` is nthr further on
            int left = n_items;          // items not yet converted, a's included
            if constexpr (BUF) {
                if (straddle) {          // one item at a time
#pragma unroll 1
                    for (; left > 0; --left, vox += nthr) {
                        load_with_pointers(a, slot(vox, a.ok));
                        convert(a, vox, has_pro, act_c);
                    }
                    return;
                }
            }
            fetch(a, vox);
#pragma unroll 1
            for (; left > 2; left -= 2, vox += 2 * nthr) {
                fetch(b, vox + nthr);
                convert(a, vox, has_pro, act_c);
                fetch(a, vox + 2 * nthr);
                convert(b, vox + nthr, has_pro, act_c);
            }
            if (left == 2) {
                fetch(b, vox + nthr);
                convert(a, vox, has_pro, act_c);
                convert(b, vox + nthr, has_pro, act_c);
            } else {
                convert(a, vox, has_pro, act_c);
            }
        };
        if (A.pro_a) {
            if (A.act == 1) pipeline(T{}, std::integral_constant<int, 1>{});
            else if (A.act == 2) pipeline(T{}, std::integral_constant<int, 2>{});
            else pipeline(T{}, std::integral_constant<int, 0>{});
        } else {
            if (A.act == 1) pipeline(F{}, std::integral_constant<int, 1>{});
            else if (A.act == 2) pipeline(F{}, std::integral_constant<int, 2>{});
            else pipeline(F{}, std::integral_constant<int, 0>{});
        }
    };
    // ---- MFMA over the taps of one chunk; the A fragments of tap t+1 are fetched during tap t ----
    auto mfma_chunk = [&](int c_base, const uint4* buf) {
        __builtin_amdgcn_s_setprio(3);   // the MFMA phase issues ahead of a co-resident workgroup's staging (+1 % measured)
        if constexpr (EX) {
            const float* ldsF = reinterpret_cast<const float*>(buf);
            const size_t tapw = (size_t)A.cin * A.coutp;                 // floats per tap
            const float* wc = wF + (size_t)c_base * A.coutp;
            float a[8][MB], an[8][MB];
#pragma unroll
            for (int kp = 0; kp < 8; ++kp)
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) a[kp][mb] = wc[(size_t)(2 * kp) * A.coutp + mb * 32];
#pragma unroll 1
            for (int zy = 0; zy < KS * KS; ++zy) {
                const int dz = zy / KS, dy = zy - dz * KS;
                const int rowoff = (dz * A.HY + dy) * A.HX;
#pragma unroll
                for (int dx = 0; dx < KS; ++dx) {
                    const int tap = zy * KS + dx;
                    const int nxt = (tap + 1 < TAPS) ? tap + 1 : tap;
#pragma unroll
                    for (int kp = 0; kp < 8; ++kp)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) an[kp][mb] = wc[(size_t)nxt * tapw + (size_t)(2 * kp) * A.coutp + mb * 32];
                    __builtin_amdgcn_sched_barrier(0);   // (as below: keep the next tap's A loads up here)
#pragma unroll
                    for (int kp = 0; kp < 8; ++kp) {
                        float b[NB];
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb) b[nb] = ldsF[voff[nb] + rowoff + dx + 2 * kp * A.CS];
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                            for (int nb = 0; nb < NB; ++nb)
                                acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[kp][mb], b[nb], acc[mb][nb], 0, 0, 0);
                    }
#pragma unroll
                    for (int kp = 0; kp < 8; ++kp)
#pragma unroll
                        for (int mb = 0; mb < MB; ++mb) a[kp][mb] = an[kp][mb];
                }
            }
            __builtin_amdgcn_s_setprio(0);
            return;
        }
        const uint4* ldsHi = buf;
        const uint4* ldsLo = buf + 2 * A.CS;
        const uint4* wh = wHi + (size_t)(c_base >> 3) * A.coutp;
        const uint4* wl = wLo + (size_t)(c_base >> 3) * A.coutp;
        if constexpr (SP) {
            // 16 steps of 2 MB MFMA triples: (ez, ey) rolled, (ex, px) unrolled; step (ez, ey, ex, px) multiplies the weights
            // of x parity px, tap (ez, ey, ex) with the tile at halo offset (ez, ey, px + ex).  As below, the A fragments of
            // the next step are fetched during this one.
            f16x8 ah[MB], al[MB];
#pragma unroll
            for (int mb = 0; mb < MB; ++mb) {
                ah[mb] = __builtin_bit_cast(f16x8, wh[mb * 32]);
                al[mb] = __builtin_bit_cast(f16x8, wl[mb * 32]);
            }
#pragma unroll 1
            for (int zy = 0; zy < 4; ++zy) {
                const int rowoff = ((zy >> 1) * A.HY + (zy & 1)) * A.HX;
                const int zyn = zy < 3 ? zy + 1 : 3;              // last step: re-read a valid fragment (harmless)
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int ex = q >> 1, px = q & 1;
                    const size_t nxt = (q < 3) ? (size_t)(((q + 1) & 1) * 8 + zy * 2 + ((q + 1) >> 1)) * tap_stride : (size_t)(zyn * 2) * tap_stride;
                    f16x8 ahn[MB], aln[MB];
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        ahn[mb] = __builtin_bit_cast(f16x8, wh[nxt + mb * 32]);
                        aln[mb] = __builtin_bit_cast(f16x8, wl[nxt + mb * 32]);
                    }
                    __builtin_amdgcn_sched_barrier(0);
                    f16x8 bh[2], bl[2];
#pragma unroll
                    for (int s = 0; s < 2; ++s) {
                        bh[s] = __builtin_bit_cast(f16x8, ldsHi[voff[px * 2 + s] + rowoff + ex]);
                        bl[s] = __builtin_bit_cast(f16x8, ldsLo[voff[px * 2 + s] + rowoff + ex]);
                    }
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            acc[mb][px * 2 + s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mb], bh[s], acc[mb][px * 2 + s], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            acc[mb][px * 2 + s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bl[s], acc[mb][px * 2 + s], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int s = 0; s < 2; ++s)
                            acc[mb][px * 2 + s] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bh[s], acc[mb][px * 2 + s], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) { ah[mb] = ahn[mb]; al[mb] = aln[mb]; }
                }
            }
            __builtin_amdgcn_s_setprio(0);
            return;
        }
        f16x8 ah[MB], al[MB];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            ah[mb] = __builtin_bit_cast(f16x8, wh[mb * 32]);
            al[mb] = __builtin_bit_cast(f16x8, wl[mb * 32]);
        }
#pragma unroll 1
        for (int zy = 0; zy < KS * KS; ++zy) {
            const int dz = zy / KS, dy = zy - dz * KS;
            const int rowoff = (dz * A.HY + dy) * A.HX;
#pragma unroll
            for (int dx = 0; dx < KS; ++dx) {
                const int tap = zy * KS + dx;
                const int nxt = (tap + 1 < TAPS) ? tap + 1 : tap;   // last tap: re-read itself (harmless)
                f16x8 ahn[MB], aln[MB];
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) {
                    ahn[mb] = __builtin_bit_cast(f16x8, wh[(size_t)nxt * tap_stride + mb * 32]);
                    aln[mb] = __builtin_bit_cast(f16x8, wl[(size_t)nxt * tap_stride + mb * 32]);
                }
                // keep the A loads of the next tap up here: left alone, the scheduler sinks them to just before their first
                // use and every tap then waits a full L2 round trip (measured: 31 us per chunk instead of 22; fetching two
                // taps ahead instead of one gains nothing more)
                __builtin_amdgcn_sched_barrier(0);
                f16x8 bh[NB], bl[NB];
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    bh[nb] = __builtin_bit_cast(f16x8, ldsHi[voff[nb] + rowoff + dx]);
                    bl[nb] = __builtin_bit_cast(f16x8, ldsLo[voff[nb] + rowoff + dx]);
                }
                // small terms first, then the leading term; every accumulator is revisited after MB*NB MFMAs
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mb], bh[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bl[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bh[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                for (int mb = 0; mb < MB; ++mb) { ah[mb] = ahn[mb]; al[mb] = aln[mb]; }
            }
        }
        __builtin_amdgcn_s_setprio(0);
    };

    float inv2 = 0.0f;   // unscale factor after a folded skip convolution
    {
        const int c_begin = A.partial ? (int)blockIdx.z * A.chunks_per_slice * 16 : 0;
        const int c_end = A.partial ? min(A.cin, c_begin + A.chunks_per_slice * 16) : A.cin;
        if constexpr (PAIR) {
            // Half-steps.  A quartet always stages its own half of a chunk's slots, [0, half) or [half, CS): at h = -1 both stage
            // chunk 0, which so is staged by all 512 threads; after that a quartet alternates between staging its half of the
            // next chunk and multiplying the chunk in hand, quartet 0 staging first, and every odd h ends in the barrier.  Chunk
            // c lives in buffer c & 1: it is written during iteration c - 1, while both quartets read buffer (c - 1) & 1, and read
            // during iteration c.
            // One copy of each phase, under two guards of their own.  Measured by cross-compilation, <3,2,4> / <3,2,2> VGPRs
            // (4-wave twins: 253 / 172): this form 249 / 175; `if (stage) ... else ...` in the same loop 256 and 244 spilled /
            // 232; a second copy of stage_chunk for chunk 0 (all threads over [0, CS)) in front of either loop 256 / 248-250 and
            // the epilogue's scalar pins no longer compile; the staging thread count and slot range as loop-carried variables
            // 253 and 244 spilled / 230.
            const int n_chunks = (c_end - c_begin) >> 4;
            const int half = (A.CS + 1) >> 1;
            const int s0 = quartet ? half : 0, s1 = quartet ? A.CS : half;
#pragma unroll 1
            for (int h = -1; h < 2 * n_chunks; ++h) {
                const int k = h >> 1;                       // the chunk in hand (-1 before the first)
                const bool stage = (h < 0 || ((h + quartet) & 1) == 0) && k + 1 < n_chunks;
                const bool multiply = h >= 0 && ((h + quartet) & 1) != 0;
                if (stage) stage_chunk(c_begin + 16 * (k + 1), smem16 + ((k + 1) & 1) * bufsz, qtid, NT, s0, s1);
                if (multiply) mfma_chunk(c_begin + 16 * k, smem16 + (k & 1) * bufsz);
                if (h & 1) __syncthreads();
            }
        } else {
        for (int c_base = c_begin; c_base < c_end; c_base += 16) {
            __syncthreads();  // previous chunk fully consumed
            stage_chunk(c_base, smem16, tid, NT, 0, A.CS);
            __syncthreads();
            mfma_chunk(c_base, smem16);
        }
        }
        if constexpr (SK != 0) {
            // ---- the block's 1x1x1 skip convolution, in the same accumulators (so that out = conv(h) + skip(x) leaves this
            // launch; the skip tensor is never written or re-read).  acc holds sum (w s_w)(x s_x); the skip products carry
            // (s_w' s_x') instead, so acc is first multiplied by (s_w' s_x') / (s_w s_x) -- a power of two, exact.
            float sb = __uint_as_float(*A.sk_amax0);
            if (A.sk_amax1) sb = fmaxf(sb, __uint_as_float(*A.sk_amax1));
            const int ex2 = scale_exponent(sb);
            const float sx2 = pow2i(ex2);
            const float inv_main = __uint_as_float(A.w16[0].x) * pow2i(-ex);
            inv2 = __uint_as_float(A.sk_w16[0].x) * pow2i(-ex2);
            const float ratio = inv_main / inv2;
#pragma unroll
            for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                    for (int r = 0; r < 16; ++r) acc[mb][nb][r] *= ratio;
            // One tap, so no LDS tile is needed: the B fragment of lane (kh, l31) in block nb is 8 channels of that lane's OWN
            // voxel, and a wave holds every c_out block of its own voxels -- a staged value is written once and read once, by the
            // lane that can load it itself.  The lane loads the 8 raw values of channels c2 + 8 kh .. + 7 per block straight from
            // sk_in0 | sk_in1 and splits them with the arithmetic of the staged form, so the products and their order are the
            // same.  No barrier, no LDS access: per chunk the 8 NB + 2 MB loads go out back to back, ONE exposed round trip
            // (staged: three, and two barriers), which the co-resident workgroup's tap loop covers.
            // Not pipelined across chunks: the forms with the next chunk's loads in flight during this chunk's MFMAs (a second
            // raw set; one raw set refilled behind the conversion; one or two A sets) all spill on <3,2,4> (246 - 1116 VGPRs) and
            // cost <1,1,2> and <1,2,2> a wave of occupancy; this one keeps every instantiation at the registers of its twin
            // without a skip.
            // Addresses: a raw buffer over the chunk's first channel, the channel as the scalar offset, the lane's voxel (+ 8
            // channels for kh = 1) as the 32-bit vector offset; the launcher checks that 16 channels span less than 4 GiB.  With
            // 64-bit lane pointers the compiler keeps an address pair per load (<3,2,4>: 414 spilled VGPRs), and it regroups
            // global loads from scalar base + lane offset into that form.
            auto sk_chunks = [&]() {
                // The lane's geometry is derived again, from copies the optimiser cannot see through: otherwise the offsets are
                // computed at the top of the kernel, next to voff[] and ovox[], and stay live across the tap loop.
                int l31s = l31, khs = kh, waves = wave;
                asm volatile("" : "+v"(l31s), "+v"(khs), "+v"(waves));
                const unsigned chb = 4u * (unsigned)ISP;     // bytes per channel
                unsigned off[NB];     // the lane's voxel and k-half in a chunk, in bytes; masked lanes read voxel 0
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    const int j = (waves * NB + nb) * 32 + l31s;
                    const int x = j & (A.TX - 1), y = (j >> A.lTX) & (A.TY - 1), z = j >> (A.lTX + A.lTY);
                    off[nb] = (valid[nb] ? 4u * (unsigned)(((oz0 + z) * A.IH + (oy0 + y)) * A.IW + ox0 + x) : 0u) + 8u * (unsigned)khs * chb;
                }
                const unsigned wlane = 16u * (unsigned)(khs * A.coutp + l31s);   // byte offset of the lane's A fragment in a k-group pair
                const char* w2Hi = reinterpret_cast<const char*>(A.sk_w16 + kW16HeaderU4 + cout0);
                const char* w2Lo = w2Hi + (size_t)(A.sk_cin >> 3) * A.coutp * sizeof(uint4);   // one tap: the lo plane follows the hi plane
#pragma unroll 1
                for (int c2 = 0; c2 < A.sk_cin; c2 += 16) {
                    f16x8 ah[MB], al[MB];
                    const size_t wrow = (size_t)(c2 >> 3) * A.coutp * sizeof(uint4);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        al[mb] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(w2Lo + wrow + mb * 32 * sizeof(uint4) + wlane));
                        ah[mb] = __builtin_bit_cast(f16x8, *reinterpret_cast<const uint4*>(w2Hi + wrow + mb * 32 * sizeof(uint4) + wlane));
                    }
                    // sk_c0 % 16 == 0 here: the chunk's 16 channels lie in one tensor
                    const float* base = (c2 < A.sk_c0) ? (A.sk_in0 + (size_t)c2 * ISP) : (A.sk_in1 + (size_t)(c2 - A.sk_c0) * ISP);
                    const __amdgpu_buffer_rsrc_t rsrc = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), 0, -1, 0x00020000);
                    float v[NB][8];
#pragma unroll
                    for (int q = 0; q < 8; ++q)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            v[nb][q] = __uint_as_float(__builtin_amdgcn_raw_buffer_load_b32(rsrc, (int)off[nb], (int)((unsigned)q * chb), 0));
                    __builtin_amdgcn_sched_barrier(0);   // all loads of the chunk ahead of the first conversion
                    f16x8 bh[NB], bl[NB];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
#pragma unroll
                        for (int q = 0; q < 8; ++q) {
                            const float sc = valid[nb] ? v[nb][q] * sx2 : 0.0f;
                            const _Float16 hq = (_Float16)sc;
                            bh[nb][q] = hq;
                            bl[nb][q] = (_Float16)(sc - (float)hq);
                        }
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mb], bh[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bl[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bh[nb], acc[mb][nb], 0, 0, 0);
                    __builtin_amdgcn_sched_barrier(0);   // the next chunk's loads reuse these registers: they stay below
                }
            };
            if constexpr (SK == 2) {
                // the parts meet inside a chunk (sk_c0 % 16 == 8; no layer of the networks): staged through LDS, as every folded skip
                // was before.  The register-fed forms of this case (a lane-valued base, or two exec-masked halves) spill on
                // <3,2,4>, and so does this loop beside the one above in one kernel: hence instantiations of its own.
                const int KG2 = A.sk_cin >> 3;
                const uint4* w2Hi = A.sk_w16 + kW16HeaderU4 + (size_t)kh * A.coutp + cout0 + l31;
                const uint4* w2Lo = w2Hi + (size_t)KG2 * A.coutp;          // one tap: the lo plane follows the hi plane
                const int centre = (KS == 3) ? (A.HY + 1) * A.HX + 1 : 0;   // LDS offset of the tile's own voxels inside the halo'd tile
                const int tvox = A.TX * A.TY * A.TZ;
                for (int c2 = 0; c2 < A.sk_cin; c2 += 16) {
                    f16x8 ah[MB], al[MB];
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb) {
                        ah[mb] = __builtin_bit_cast(f16x8, w2Hi[(size_t)(c2 >> 3) * A.coutp + mb * 32]);
                        al[mb] = __builtin_bit_cast(f16x8, w2Lo[(size_t)(c2 >> 3) * A.coutp + mb * 32]);
                    }
                    __syncthreads();   // previous chunk fully consumed
                    uint4* bHi = smem16;
                    uint4* bLo = smem16 + 2 * A.CS;
                    for (int j = tid; j < tvox; j += NT) {   // raw values, interior voxels only (one tap: no halo)
                        const int x = j & (A.TX - 1), y = (j >> A.lTX) & (A.TY - 1), z = j >> (A.lTX + A.lTY);
                        const bool okv = (ox0 + x < A.OW) && (oy0 + y < A.OH) && (oz0 + z < A.OD);
                        const size_t sidx = okv ? ((size_t)(oz0 + z) * A.IH + (oy0 + y)) * A.IW + ox0 + x : 0;
                        float val[16];
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const int cg = c2 + q;
                            const float* src = (cg < A.sk_c0) ? (A.sk_in0 + (size_t)cg * ISP) : (A.sk_in1 + (size_t)(cg - A.sk_c0) * ISP);
                            val[q] = src[sidx];
                        }
                        f16x8 vh[2], vl[2];
#pragma unroll
                        for (int q = 0; q < 16; ++q) {
                            const float sc = okv ? val[q] * sx2 : 0.0f;
                            const _Float16 hq = (_Float16)sc;
                            vh[q >> 3][q & 7] = hq;
                            vl[q >> 3][q & 7] = (_Float16)(sc - (float)hq);
                        }
                        const int slot = (z * A.HY + y) * A.HX + x + centre;
                        bHi[slot] = __builtin_bit_cast(uint4, vh[0]);
                        bHi[A.CS + slot] = __builtin_bit_cast(uint4, vh[1]);
                        bLo[slot] = __builtin_bit_cast(uint4, vl[0]);
                        bLo[A.CS + slot] = __builtin_bit_cast(uint4, vl[1]);
                    }
                    __syncthreads();
                    f16x8 bh[NB], bl[NB];
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb) {
                        bh[nb] = __builtin_bit_cast(f16x8, bHi[voff[nb] + centre]);
                        bl[nb] = __builtin_bit_cast(f16x8, bLo[voff[nb] + centre]);
                    }
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(al[mb], bh[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bl[nb], acc[mb][nb], 0, 0, 0);
#pragma unroll
                    for (int mb = 0; mb < MB; ++mb)
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            acc[mb][nb] = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah[mb], bh[nb], acc[mb][nb], 0, 0, 0);
                }
            } else {
                sk_chunks();
            }
        }
    }

    // ---- epilogue: unscale, + bias (+ residual); C/D layout: column = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) ----
    // With A.stats the statistics the NEXT layer's LayerNorm/GroupNorm needs are taken here, while the values are in
    // registers: per output channel the sum and sum of squares over this workgroup's voxels (lane -> 32-lane DPP
    // reduction -> 4 waves through LDS) go to stats[tile][c_out_padded][2] with plain stores, and the tile's |x|max
    // to *out_amax; pixie_stats_finalize adds the tiles up in fp64.  That replaces one full read of the tensor.
    const float inv = EX ? 1.0f : (SK != 0 ? inv2 : __uint_as_float(A.w16[0].x) * pow2i(-ex));
    if (A.partial) {   // split-K slice: raw partial sums; bias, residual and statistics belong to splitk_reduce_kernel
        float* dst = A.partial + (size_t)blockIdx.z * A.cout * OSP;
#pragma unroll
        for (int mb = 0; mb < MB; ++mb)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int co = cout0 + mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
                if (co < A.cout) {
#pragma unroll
                    for (int nb = 0; nb < NB; ++nb)
                        if (valid[nb]) dst[(size_t)co * OSP + ovox[nb]] = acc[mb][nb][r] * inv;
                }
            }
        return;
    }
    // [4 waves][MB*32 rows][2], reused after the last chunk.  Pair form: one such array per quartet, behind the eight waves'
    // transposing area where the launch reserved one -- the quartets of a tile may take different epilogue paths (a partly padded
    // second block), so the place cannot depend on the path.
    constexpr int LDO_ = NB * 32 + 4;
    float* red = reinterpret_cast<float*>(smem16) + (PAIR ? (A.epi_lds ? 2 * NW * 32 * LDO_ : 0) + quartet * (NW * MB * 64) : 0);
    float wmax = 0.0f;
    // workgroup-uniform: every accumulator element of this tile is a real output
    const bool full = SP ? (A.epi_lds && cout0 + MB * 32 <= A.cout && (A.TX & 1) == 0 && (A.OW & 3) == 0 && NW * 64 <= A.TX * A.TY * A.TZ &&
                            2 * (ox0 + A.TX) <= A.OW && 2 * (oy0 + A.TY) <= A.OH && 2 * (oz0 + A.TZ) <= A.OD)
                         : (A.epi_lds && cout0 + MB * 32 <= A.cout && (A.TX & 3) == 0 && (A.OW & 3) == 0 && NW * NB * 32 <= A.TX * A.TY * A.TZ &&
                            ox0 + A.TX <= A.OW && oy0 + A.TY <= A.OH && oz0 + A.TZ <= A.OD);
    if (full) {
        // Interior tile (every tile of the 128^3 layers).  The accumulators go through LDS (the activation tile is dead)
        // so that each lane ends up with 4 x-consecutive voxels of one row: 16-byte residual loads and stores, 8x fewer
        // memory instructions than from the MFMA register layout.  (Written naively from that layout, every residual load
        // carried an s_waitcnt vmcnt(0) that also drained the preceding store: 256 serialised memory round trips, 42 us
        // of a 229 us workgroup.  The first transposing version still had one such round trip per ROW: runtime branches
        // around the bias and residual loads kept the rows serial, and gfx9's single in-order vmcnt made each row's loads
        // wait for the previous row's store.  Now no load waits behind a store: the bias is fetched once per block, ahead
        // of the barrier, the residual a group of four rows ahead of the stores, and (residual, statistics) select one of
        // four straight-line bodies.)
        constexpr int LDO = NB * 32 + 4;                                  // row stride in floats
        float* ldsO = reinterpret_cast<float*>(smem16) + (quartet * NW + wave) * (32 * LDO);   // this wave's 32 rows; no other wave touches it
        if constexpr (!PAIR) red = reinterpret_cast<float*>(smem16) + NW * 32 * LDO;
        constexpr int LPR = NB * 8;          // lanes per row (4 voxels each)
        constexpr int RPI = 32 / LPR;        // rows per half-wave per iteration
        constexpr int NIT = 16 / RPI;        // rows of a 32-row block this lane takes
        constexpr int G = 4;                 // rows per group: the residual of group q + 1 is in flight during the stores of group q
        constexpr int GPB = NIT / G;         // groups per block
        constexpr int NGRP = MB * GPB;
        const int rsub = l31 / LPR, colq = 4 * (l31 % LPR), nbq = colq >> 5;
        // bias (+ folded-skip bias): lane l fetches that of row l & 31 of each block, here, ahead of the barrier; it is added in
        // the MFMA layout on the way into LDS, where a lane's 16 rows of a block are compile-time lanes (+ 4 kh): v_readlane, no
        // loads in the row code.  A missing bias is read from the weight array instead (any cout readable floats) and replaced
        // by 0 afterwards, so the loads need no branch.
        const float* nobias = EX ? A.wf : reinterpret_cast<const float*>(A.w16);
        const bool hb0 = A.bias != nullptr, hb1 = A.sk_bias != nullptr;
        float braw[MB][2];
#pragma unroll
        for (int mb = 0; mb < MB; ++mb) {
            braw[mb][0] = (hb0 ? A.bias : nobias)[cout0 + mb * 32 + l31];
            braw[mb][1] = (hb1 ? A.sk_bias : nobias)[cout0 + mb * 32 + l31];
        }
        __syncthreads();   // every wave is done with the activation tile
        // SP: column 2 j + px of a wave's row is x parity px of its stored voxel j, so 4 columns are 4 x-consecutive outputs
        const int jq = SP ? wave * 64 + (colq >> 1) : (wave * NB + nbq) * 32 + (colq & 31);
        const int xq = jq & (A.TX - 1), yq = (jq >> A.lTX) & (A.TY - 1), zq = jq >> (A.lTX + A.lTY);
        const size_t ovq = SP ? ((size_t)(2 * (oz0 + zq) + pz) * A.OH + (2 * (oy0 + yq) + py)) * A.OW + 2 * (ox0 + xq)
                              : ((size_t)(oz0 + zq) * A.OH + (oy0 + yq)) * A.OW + ox0 + xq;
        // The lane's rows, block after block, are local rows (2 it + kh) RPI + rsub: 2 RPI channels apart, also across the
        // blocks (2 RPI NIT = 32), so one running pointer each for the residual (fetched ahead) and the output.
        const size_t orow0 = (size_t)(cout0 + kh * RPI + rsub) * OSP + ovq;
        auto rows = [&](auto res_c, auto stats_c) {
            constexpr bool RES = decltype(res_c)::value, STATS = decltype(stats_c)::value;
            // The step is opaque to the optimiser: otherwise the 64-bit addresses of all 2 x 32 rows, the same in the four
            // bodies, are computed ahead of the dispatch and held in 128 VGPRs (spilled) instead of two running pointers.
            size_t step = (size_t)(2 * RPI) * OSP;
            asm volatile("" : "+s"(step));
            const float* pr = A.residual + orow0;
            float* po = A.out + orow0;
            float4 r4[2][G];     // residual of the group in hand and of the next one
            auto fetch = [&](int q) {
#pragma unroll
                for (int g = 0; g < G; ++g) { r4[q & 1][g] = *reinterpret_cast<const float4*>(pr); pr += step; }
            };
#pragma unroll
            for (int q = 0; q < NGRP; ++q) {
                const int mb = q / GPB, it0 = (q % GPB) * G;
                // A group's loads and stores stay in their group.  (Left free, the scheduler pulls the residual of many groups
                // ahead in the bodies without statistics and spills; amdgcn_sched_barrier here, or groups of 8 rows, or a second
                // group in flight spill too: the tap loop leaves these kernels at 254 VGPRs.)
                asm volatile("" ::: "memory");
                if (q % GPB == 0) {
                    const int brow = __float_as_int((hb0 ? braw[mb][0] : 0.0f) + (hb1 ? braw[mb][1] : 0.0f));
#pragma unroll
                    for (int r = 0; r < 16; ++r) {
                        const int row = (r & 3) + 8 * (r >> 2);
                        const int blo = __builtin_amdgcn_readlane(brow, row), bhi = __builtin_amdgcn_readlane(brow, row + 4);
                        const float bv = __int_as_float(kh ? bhi : blo);
#pragma unroll
                        for (int nb = 0; nb < NB; ++nb)
                            ldsO[((r & 3) + 8 * (r >> 2) + 4 * kh) * LDO + (SP ? 2 * ((nb & 1) * 32 + l31) + (nb >> 1) : nb * 32 + l31)] =
                                __builtin_fmaf(acc[mb][nb][r], inv, bv);
                    }
                }
                if constexpr (RES) {
                    if (q == 0) fetch(0);      // behind block 0's LDS writes: while both blocks' accumulators are live there is no room for it
                    if (q + 1 < NGRP) fetch(q + 1);
                }
                float4 v4[G];
#pragma unroll
                for (int g = 0; g < G; ++g) {
                    const int rowl = (2 * (it0 + g) + kh) * RPI + rsub;
                    v4[g] = *reinterpret_cast<const float4*>(ldsO + rowl * LDO + colq);
                    if constexpr (RES) { v4[g].x += r4[q & 1][g].x; v4[g].y += r4[q & 1][g].y; v4[g].z += r4[q & 1][g].z; v4[g].w += r4[q & 1][g].w; }
                    *reinterpret_cast<float4*>(po) = v4[g]; po += step;
                }
                if constexpr (STATS) {
                    // per row the xor butterfly over its LPR lanes, as before; the G rows' chains are independent and interleaved
                    float s1[G], s2[G];
#pragma unroll
                    for (int g = 0; g < G; ++g) {
                        const float4 v = v4[g];
                        s1[g] = (v.x + v.y) + (v.z + v.w);
                        s2[g] = (v.x * v.x + v.y * v.y) + (v.z * v.z + v.w * v.w);
                        wmax = fmaxf(fmaxf(wmax, fmaxf(fabsf(v.x), fabsf(v.y))), fmaxf(fabsf(v.z), fabsf(v.w)));
                    }
                    asm volatile("" : "+v"(wmax));   // taken here: left to the optimiser, the max is sunk below the last row and every output stays live (spills)
#pragma unroll
                    for (int off = LPR / 2; off > 0; off >>= 1) {
                        float t1[G], t2[G];
#pragma unroll
                        for (int g = 0; g < G; ++g) { t1[g] = __shfl_xor(s1[g], off, 64); t2[g] = __shfl_xor(s2[g], off, 64); }
#pragma unroll
                        for (int g = 0; g < G; ++g) { s1[g] += t1[g]; s2[g] += t2[g]; }
                    }
                    if ((l31 % LPR) == 0) {
#pragma unroll
                        for (int g = 0; g < G; ++g) {
                            const int rowl = (2 * (it0 + g) + kh) * RPI + rsub;
                            red[(wave * MB * 32 + mb * 32 + rowl) * 2] = s1[g]; red[(wave * MB * 32 + mb * 32 + rowl) * 2 + 1] = s2[g];
                        }
                    }
                }
            }
        };
        using T = std::true_type; using F = std::false_type;
        if (A.residual) { if (A.stats) rows(T{}, T{}); else rows(T{}, F{}); }
        else { if (A.stats) rows(F{}, T{}); else rows(F{}, F{}); }
    } else {
    if (PAIR || A.stats) __syncthreads();            // every wave is done with the activation tile (pair form: the other quartet may be on the path above, with its barrier)
#pragma unroll
    for (int mb = 0; mb < MB; ++mb) {
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int row = mb * 32 + (r & 3) + 8 * (r >> 2) + 4 * kh;
            const int co = cout0 + row;
            float s1 = 0.0f, s2 = 0.0f;
            if (co < A.cout) {
                const float bv = (A.bias ? A.bias[co] : 0.0f) + (A.sk_bias ? A.sk_bias[co] : 0.0f);
#pragma unroll
                for (int nb = 0; nb < NB; ++nb) {
                    if (valid[nb]) {
                        const size_t o = (size_t)co * OSP + ovox[nb];
                        float val = acc[mb][nb][r] * inv + bv;
                        if (A.residual) val += A.residual[o];
                        A.out[o] = val;
                        s1 += val; s2 += val * val; wmax = fmaxf(wmax, fabsf(val));
                    }
                }
            }
            if (A.stats) {
#pragma unroll
                for (int off = 16; off > 0; off >>= 1) { s1 += __shfl_xor(s1, off, 64); s2 += __shfl_xor(s2, off, 64); }
                if (l31 == 0) { red[(wave * MB * 32 + row) * 2] = s1; red[(wave * MB * 32 + row) * 2 + 1] = s2; }
            }
        }
    }
    }
    if (A.stats) {
        __syncthreads();
        if (qtid < MB * 32 * 2) {
            float t = red[qtid];
#pragma unroll
            for (int w = 1; w < NW; ++w) t += red[w * MB * 64 + qtid];      // fixed order
            A.stats[((size_t)blockIdx.x * A.coutp + cout0) * 2 + qtid] = t;
        }
        if (A.out_amax) {
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) wmax = fmaxf(wmax, __shfl_xor(wmax, off, 64));
            if (lane == 0 && wmax > 0.0f) atomicMax(A.out_amax, __float_as_uint(wmax));
        }
    }
}

template <int KS, int MB, int NB>
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_kernel(Conv16Args A) {
    conv3d_f16x3_body<KS, MB, NB>(A);
}
// Pair form: 8 waves over one tile and two 64-channel blocks (see the body); one workgroup per CU, the same 8 waves as two 4-wave ones
template <int KS, int NB>
__global__ __launch_bounds__(512, 1) void conv3d_f16x3_pair_kernel(Conv16Args A) {
    conv3d_f16x3_body<KS, 2, NB, false, false, 0, true>(A);
}
// The same launch with a folded 1x1x1 skip convolution (SK): instantiations of their own, so that the skip loop's registers are
// not charged to the kernels that never run it (the sub-pixel path got the same treatment).  conv_plan() can answer
// skip_foldable with every <KS, MB, NB> of the variant table (without a workspace a small output shrinks NB, then MB), so the
// table is instantiated whole.
// STAGED: the skip's parts meet inside a 16-channel chunk (skip_c0 % 16 == 8), see the body.
template <int KS, int MB, int NB, bool STAGED>
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_skip_kernel(Conv16Args A) {
    conv3d_f16x3_body<KS, MB, NB, false, false, STAGED ? 2 : 1>(A);
}
// conv_precision = "f32": the exact-fp32 variant of the same body (v_mfma_f32_32x32x2_f32)
template <int KS, int MB, int NB>
__global__ __launch_bounds__(256, 2) void conv3d_exact_kernel(Conv16Args A) {
    conv3d_f16x3_body<KS, MB, NB, true>(A);
}
// Sub-pixel form of the 3^3 convolutions behind a nearest x2 upsampling (Upsample.conv): 8 taps per output instead of 27
template <int MB>
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_subpixel_kernel(Conv16Args A) {
    conv3d_f16x3_body<3, MB, 4, false, true>(A);
}
// The dominant layer of the BASELINE network -- 64 -> 64 channels, 3^3, stride 1, on >= 128^3 voxels (the full-resolution
// level: 41 % of a scene's FLOPs at 128^3; the 64^3 level has the same channel counts and stays on the template) -- under its own symbol, so that `rocprofv3 --kernel-trace --stats` reports it as
// its own row instead of pooling it with the other shapes that share the <3,2,4> instantiation.  Same code, same results.
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_c64_fullres_kernel(Conv16Args A) {
    conv3d_f16x3_body<3, 2, 4>(A);
}

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
constexpr int kReduceSeg = 4096;
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

// split-K launches: segments per channel of splitk_reduce_stats_kernel = partial statistics per channel
static int reduce_segments(long osp) { return (int)((osp + kReduceSeg - 1) / kReduceSeg); }

bool conv_exact_v1() { return getenv("PIXIE_CONV_EXACT_V1") != nullptr; }

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

// the output dims of a convolution: padding ksize / 2, nearest x2 upsampling first, cropped to out_* where given
static void conv_output_dims(const ConvShape& s, int& od, int& oh, int& ow) {
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
ConvPlan conv_plan(const ConvShape& s) {
    ConvPlan p;
    auto refuse = [&p](ConvRefusal why) { p.path = CONV_NONE; p.refusal = why; return p; };
    if ((s.ksize != 1 && s.ksize != 3) || (s.stride != 1 && s.stride != 2) || (s.upsample != 0 && s.upsample != 1) || s.c0 <= 0 || s.c1 < 0 ||
        s.c_out <= 0 || s.in_d <= 0 || s.in_h <= 0 || s.in_w <= 0)
        return refuse(CONV_BAD_SHAPE);
    conv_output_dims(s, p.OD, p.OH, p.OW);
    p.KS = s.ksize; p.coutp = pixie_conv_cout_padded(s.c_out);
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
    p.lds_bytes = (size_t)4 * p.CS * sizeof(uint4);   // four 16-byte fp16 planes per halo voxel (exact: 16 fp32 planes)
    if (p.lds_bytes > 160 * 1024) return refuse(CONV_BAD_LDS);
    // LDS the transposing epilogue needs (4 waves x 32 rows x (NB*32 + 4) floats + the statistics partials), and whether the launch
    // gets it: unsplit launches only, as long as two workgroups still fit on a CU
    const size_t epi_bytes = ((size_t)4 * 32 * (p.NB * 32 + 4) + (size_t)4 * p.MB * 32 * 2) * sizeof(float);
    if (p.slices == 1 && epi_bytes <= 80 * 1024) { p.epi_lds = 1; p.lds_bytes = std::max(p.lds_bytes, epi_bytes); }
    p.grid = dim3((unsigned)p.n_tiles, (unsigned)((p.coutp + p.MB * 32 - 1) / (p.MB * 32)), (unsigned)p.slices);
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

// The pair form of a planned launch (conv3d_f16x3_pair_kernel): the same plan -- tile, MB, NB, variant number, statistics layout
// -- launched with 512 threads over (n_tiles, coutp / 128).  A pure function of the plan and of whether a folded skip rides
// along: the plain f16x3 path, MB = 2, an even number of 64-channel blocks, and two tile buffers (or the eight waves' transposing
// epilogue area and statistics partials) within the 160 KB of a CU, which excludes every stride-2 tile.  Unsplit NB = 4 launches
// only: those are the classes that cleared the 2 % bar against their 4-wave form (profiles/conv_pair_pricing.txt: the 128^3
// launches -9.8 % and -18.3 %; the split-K launches of the 32^3 and 16^3 levels -1.1 % .. +4.8 %, so they keep the 4-wave kernels,
// and no launch of the networks reaches NB < 4 unsplit with 128 channels).  Returns the launch's dynamic LDS bytes, 0 = the launch
// keeps the 4-wave kernel.
#ifdef PIXIE_DIAG
static int g_conv_keep_four_wave = 0;   // diagnostic switch (pixie_conv_kernel_variant with a null descriptor)
#endif
static size_t conv_pair_lds(const ConvPlan& p, bool skip) {
#ifdef PIXIE_DIAG
    if (g_conv_keep_four_wave) return 0;
#endif
    if (p.path != CONV_F16X3 || p.fullres || skip || p.MB != 2 || p.NB != 4 || p.slices != 1 || p.coutp % 128 != 0) return 0;
    const size_t tiles = (size_t)2 * 4 * p.CS * sizeof(uint4);
    const size_t red = (size_t)2 * 4 * p.MB * 32 * 2 * sizeof(float);
    const size_t epi = p.epi_lds ? (size_t)8 * 32 * (p.NB * 32 + 4) * sizeof(float) + red : red;
    const size_t lds = std::max(tiles, epi);
    return lds <= 160 * 1024 ? lds : 0;
}
static ConvKernel conv16_pair_kernel(const ConvPlan& p) {
#define PX_CONV16_PAIR(KS_, NB_) \
    if (p.KS == KS_ && p.NB == NB_) return conv3d_f16x3_pair_kernel<KS_, NB_>;
    PX_CONV16_PAIR(3, 4) PX_CONV16_PAIR(1, 4)
#undef PX_CONV16_PAIR
    return nullptr;
}

static int launch(ConvKernel kern, const ConvPlan& p, const Conv16Args& a, hipStream_t st, size_t pair_lds = 0) {
    PX_REQUIRE(kern != nullptr, "conv: no kernel variant for ksize=%d MB=%d NB=%d", p.KS, p.MB, p.NB);
    PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(kern)));
    if (pair_lds) hipLaunchKernelGGL(kern, dim3(p.grid.x, p.grid.y / 2, 1), dim3(512), pair_lds, st, a);
    else hipLaunchKernelGGL(kern, p.grid, dim3(256), p.lds_bytes, st, a);
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
    if (int rc = launch(pair_lds ? conv16_pair_kernel(p) : conv16_kernel(p, a.sk_w16 != nullptr, a.sk_c0), p, a, st, pair_lds)) return rc;
    if (p.slices == 1) return 0;
    const long osp = (long)a.OD * a.OH * a.OW, n_elems = (long)a.cout * osp;
    if (d->d_out_stats) {
        const dim3 rgrid((unsigned)reduce_segments(osp), (unsigned)a.cout);
        double* rstats = reinterpret_cast<double*>(d->d_out_stats);
        PX_REQUIRE((reinterpret_cast<size_t>(rstats) & 7) == 0, "f16x3 conv: d_out_stats of a split-K launch must be 8-byte aligned");
        const bool vec = osp % 4 == 0 && ((reinterpret_cast<size_t>(a.partial) | reinterpret_cast<size_t>(a.residual) | reinterpret_cast<size_t>(a.out)) & 15) == 0;
        if (vec) hipLaunchKernelGGL(splitk_reduce_stats_kernel<true>, rgrid, dim3(256), 0, st, a.partial, p.slices, n_elems, osp, a.bias, a.residual,
                                    a.out, rstats, d->d_out_amax);
        else hipLaunchKernelGGL(splitk_reduce_stats_kernel<false>, rgrid, dim3(256), 0, st, a.partial, p.slices, n_elems, osp, a.bias, a.residual,
                                a.out, rstats, d->d_out_amax);
    } else {
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, st, a.partial, p.slices, n_elems, osp,
                           a.bias, a.residual, a.out);
    }
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

// called by pixie_conv3d_forward (conv3d_mfma.hip) for exact-fp32 descriptors (d_w, no d_w16) that the plan sends through the
// tiled body above instead of the first-generation kernel
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
    if (!p.f16x3()) return 0;
    if (p.path == CONV_F16X3_SUBPIXEL) return 8300 + p.MB * 10 + p.NB;   // conv3d_f16x3_subpixel_kernel<MB>
    if (p.fullres) return 9324;                                           // conv3d_f16x3_c64_fullres_kernel
    return p.KS * 100 + p.MB * 10 + p.NB;
}

// the tiling pixie_conv3d_forward launches this descriptor with: out = TX, TY, TZ, tiles_x, tiles_y, tiles_z, epi_lds, slices,
// MB, NB.  With d_w16 the f16x3 launch (sub-pixel: the tile lies over the STORED voxels, each tile is four workgroups);
// without, the exact-fp32 launch of the same body.  Returns 1 (and leaves out alone) for descriptors that take neither.
extern "C" int pixie_conv_tile_geometry(const pixie_conv_desc* d, int32_t out[10]) {
    const ConvPlan p = plan_of(d);
    if (!out && d) return (int)conv_pair_lds(p, d->d_skip_w16 != nullptr);   // the launcher's form for this descriptor, as it is switched now
    if (!out || !p.tiled()) return 1;
    const int32_t v[10] = {p.TX, p.TY, p.TZ, p.tiles_x, p.tiles_y, p.tiles_z, p.epi_lds, p.slices, p.MB, p.NB};
    for (int i = 0; i < 10; ++i) out[i] = v[i];
    return 0;
}

// where this descriptor's launch leaves its partial statistics, as pixie_stats_finalize / pixie_stats_norm_finalize will read them:
// out = partials per channel, cstride, tstride (in (sum, sum of squares) pairs), 1 = fp64 reduce segments /
// 0 = fp32 tile partials, voxels per reduce segment (0 for tile partials), c_out padded.  Returns 1 off the f16x3 path.
extern "C" int pixie_conv_stats_layout(const pixie_conv_desc* d, int64_t out[6]) {
    const ConvPlan p = plan_of(d);
    if (!out || !p.f16x3()) return 1;
    out[0] = p.stats.n; out[1] = p.stats.cstride; out[2] = p.stats.tstride; out[3] = p.stats.f64; out[4] = p.stats.f64 ? kReduceSeg : 0;
    out[5] = p.coutp;
    return 0;
}
#endif

extern "C" int pixie_conv_skip_foldable(const pixie_conv_desc* d) { return plan_of(d).skip_foldable ? 1 : 0; }

extern "C" int pixie_stats_finalize(const float* d_stats, const pixie_conv_desc* d, double* d_sums, void* stream) {
    PX_REQUIRE(d_stats && d && d_sums, "pixie_stats_finalize: null argument");
    // the tile (or segment) count comes from the plan conv3d_f16x3_forward launched with
    hipLaunchKernelGGL(stats_finalize_kernel, dim3((unsigned)d->c_out), dim3(256), 0, as_stream(stream), stat_parts(plan_of(d), d_stats), d_sums);
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
    hipLaunchKernelGGL(stats_norm_finalize_kernel, dim3((unsigned)(mode == 0 ? channels : groups)), dim3(256), 0, as_stream(stream), p0, d_sums0, c0,
                       p1, d_sums1, channels, (double)spatial, mode, groups, eps, d_weight, d_bias, d_a, d_b);
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
