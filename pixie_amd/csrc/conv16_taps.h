// pixie_amd/csrc/conv16_taps.h -- FRAGMENT of conv3d_f16x3_body (conv16_body.h), included inside it right after conv16_stage.h: the
// tap loop, as the lambda  mfma_chunk(c_base, buf).  No include guard: included once.
// It multiplies the staged chunk in `buf` (channels c_base .. c_base + 15) with that chunk's weights of every tap and adds the
// products to the accumulators: three f16 MFMAs per product (al.bh, ah.bl, ah.bh), or one fp32 MFMA per channel pair under EX; the
// sub-pixel form (SP) walks 2 x 2 x 2 taps for both x parities.  The A fragments of the next tap are fetched during this one.
//   template parameters read:  EX, SP, KS, MB, NB
//   names of the body read:    A, TAPS, tap_stride, voff (the lane's LDS slot per voxel block, kh folded in), wHi, wLo (f16x3) and
//                              wF (EX): the lane's weight pointers at chunk 0, with kh, l31, cout0 and the SP parity folded in
//   writes:                    acc
//   barriers:                  none inside.  `buf` is complete (a barrier behind stage_chunk) and stays untouched until every wave
//                              that reads it has left this call (a barrier in front of the next staging of the same buffer).  Runs
//                              at s_setprio 3 and returns at 0.
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
