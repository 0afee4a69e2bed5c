// pixie_amd/csrc/conv16_body.h -- the tiled convolution body conv3d_f16x3_body<KS, MB, NB, EX, SP, SK, PAIR> and its six __global__
// entry points.  The body is one function; its phases are read here in order and live in four fragments that are #included INSIDE
// it, each with its contract (template parameters and names of this scope it reads, what it writes, its barriers) at its top:
//   geometry, input scale, accumulators, weight pointers      below
//   stage_chunk(c_base, buf, stid, nthr, s0, s1)              conv16_stage.h     global -> prologue -> fp16 hi/lo planes in LDS
//   mfma_chunk(c_base, buf)                                   conv16_taps.h      the tap loop: LDS B x L2 A -> acc
//   the chunk loop (4-wave form, or the pair form's half-steps) below, calling the two
//   the folded 1x1x1 skip convolution (SK != 0)               conv16_skip.h      more products into acc; sets inv2
//   the epilogue                                              conv16_epilogue.h  acc -> out / split-K partial, statistics
// Textual inclusion, not __device__ functions: the fragments' statements are exactly the ones the body held as one file, and the
// gfx950 code object is byte for byte the same (profiles/conv_split_device_identity.txt).  The same statements behind a
// __forceinline__ function with array-reference arguments compile to different code ("Convolution file map").  A
// fragment has no include guard and is included once.
#pragma once
#include <type_traits>

#include "conv16_device.h"
#include "launch_record.h"

namespace pixie {

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
// GRP ("grouped twin", launch_list.h): the launch carries two argument sets behind a doubled grid z; A is the set of this workgroup
// and the split-K slice index is blockIdx.z within its half.  Everything else is the single form's, statement for statement.
template <int KS, int MB, int NB, bool EX = false, bool SP = false, int SK = 0, bool PAIR = false, bool GRP = false>
__device__ __forceinline__ void conv3d_f16x3_body(const Conv16Args& A) {
    static_assert(!PAIR || (MB == 2 && !EX && !SP && SK == 0), "pair form: the plain f16x3 body with 64 c_out per quartet");
    static_assert(!SP || (KS == 3 && NB == 4 && !EX), "sub-pixel path: 3^3, two x parities x two voxel blocks per wave");
    static_assert(SK == 0 || (!EX && !SP), "folded skip (SK: 1 register-fed, 2 staged through LDS): f16x3, no sub-pixel form");
    extern __shared__ uint4 smem16[];
    constexpr int PAD = (KS == 3) ? 1 : 0;
    constexpr int NW = 4, NT = 64 * NW;     // (an 8-wave, one-workgroup-per-CU tile was measured in round 4: 1.350 vs 1.323 ms, profiles/r4k_conv_eight_wave_tile_rejected.txt)
    const int bufsz = 4 * A.CS;            // one buffer: hi[2][CS], lo[2][CS]

    const unsigned zslice = GRP ? blockIdx.z - (blockIdx.z >= (gridDim.z >> 1) ? (gridDim.z >> 1) : 0u) : blockIdx.z;   // split-K slice
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
    // ---- the two phases of a chunk, as lambdas: stage_chunk(c_base, buf, stid, nthr, s0, s1) and mfma_chunk(c_base, buf) ----
#include "conv16_stage.h"
#include "conv16_taps.h"

    // ---- the chunk loop, then the folded skip convolution where the kernel has one ----
    float inv2 = 0.0f;   // unscale factor after a folded skip convolution
    {
        const int c_begin = A.partial ? (int)zslice * A.chunks_per_slice * 16 : 0;
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
#include "conv16_skip.h"
    }

#include "conv16_epilogue.h"
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
// STAGED: the skip's parts meet inside a 16-channel chunk (skip_c0 % 16 == 8), see conv16_skip.h.
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
// Grouped twins (launch_list.h, pixie_unet_forward_pair): the launches of two networks that run the same instantiation on the same
// grid, as one launch.  Workgroups with blockIdx.z in the upper half of the grid take the second argument set (wave-uniform, the
// arguments stay scalar loads from the kernel argument segment); blockIdx.x and blockIdx.y mean what they mean in the single form.
// Instantiations of their own, like the skip kernels: the single forms' code is not touched.  Which launches have one is
// conv16_group_kernel()'s table (conv3d_f16x3.hip).
template <int KS, int MB, int NB>
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_group_kernel(Group2<Conv16Args> G) {
    conv3d_f16x3_body<KS, MB, NB, false, false, 0, false, true>(G.a[blockIdx.z >= (gridDim.z >> 1) ? 1 : 0]);
}
template <int MB>
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_subpixel_group_kernel(Group2<Conv16Args> G) {
    conv3d_f16x3_body<3, MB, 4, false, true, 0, false, true>(G.a[blockIdx.z >= (gridDim.z >> 1) ? 1 : 0]);
}
// The dominant layer of the BASELINE network -- 64 -> 64 channels, 3^3, stride 1, on >= 128^3 voxels (the full-resolution
// level: 41 % of a scene's FLOPs at 128^3; the 64^3 level has the same channel counts and stays on the template) -- under its own symbol, so that `rocprofv3 --kernel-trace --stats` reports it as
// its own row instead of pooling it with the other shapes that share the <3,2,4> instantiation.  Same code, same results.
__global__ __launch_bounds__(256, 2) void conv3d_f16x3_c64_fullres_kernel(Conv16Args A) {
    conv3d_f16x3_body<3, 2, 4>(A);
}

}  // namespace pixie
