// pixie_amd/csrc/conv16_epilogue.h -- FRAGMENT of conv3d_f16x3_body (conv16_body.h), included inside it as its last statements: the
// epilogue.  No include guard: included once.
// acc -> unscale, + bias (+ folded-skip bias) (+ residual) -> A.out; or, in a split-K slice (A.partial), the raw unscaled sums ->
// A.partial[zslice], after which the fragment RETURNS from the body.  With A.stats it leaves the per-channel partial sums of
// this tile in A.stats and the tile's |x|max in *A.out_amax.  Interior tiles with the LDS reserved (A.epi_lds) transpose the
// accumulators through LDS into rows of 4 x-consecutive voxels per lane (`full`); every other tile stores from the MFMA layout.
//   template parameters read:  EX, SP, SK, PAIR, MB, NB
//   names of the body read:    A, acc, ex, inv2 (SK != 0), NW, smem16, cout0, OSP, valid, ovox, lane, l31, kh, wave, quartet, qtid,
//                              ox0, oy0, oz0, py, pz, zslice
//   writes:                    global memory (A.out or A.partial, A.stats, *A.out_amax); LDS: the activation tile is dead and
//                              reused for the transposing area and the statistics partials `red`
//   barriers:                  `full` path: one, before the first LDS write (every wave is done with the tile).  Other path: one
//                              if PAIR || A.stats.  With A.stats one more, between the waves' partials and their sum.  All are
//                              workgroup-uniform: in the pair form the quartets may take different paths, each with one barrier.
    // ---- epilogue: unscale, + bias (+ residual); C/D layout: column = lane&31, row = (r&3) + 8*(r>>2) + 4*(lane>>5) ----
    // With A.stats the statistics the NEXT layer's LayerNorm/GroupNorm needs are taken here, while the values are in
    // registers: per output channel the sum and sum of squares over this workgroup's voxels (lane -> 32-lane DPP
    // reduction -> 4 waves through LDS) go to stats[tile][c_out_padded][2] with plain stores, and the tile's |x|max
    // to *out_amax; pixie_stats_finalize adds the tiles up in fp64.  That replaces one full read of the tensor.
    const float inv = EX ? 1.0f : (SK != 0 ? inv2 : __uint_as_float(A.w16[0].x) * pow2i(-ex));
    if (A.partial) {   // split-K slice: raw partial sums; bias, residual and statistics belong to splitk_reduce_kernel
        float* dst = A.partial + (size_t)zslice * A.cout * OSP;
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
