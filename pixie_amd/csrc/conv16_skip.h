// pixie_amd/csrc/conv16_skip.h -- FRAGMENT of conv3d_f16x3_body (conv16_body.h), included inside it behind the chunk loop, in the
// loop's block: the folded 1x1x1 skip convolution, one `if constexpr (SK != 0)` statement.  No include guard: included once.
// After the main convolution's chunks it rescales the accumulators by an exact power of two and adds the products of A.sk_cin
// more channels of the RAW tensors sk_in0 | sk_in1 through the centre tap, with their own packed weights and input scale.
// SK = 1: B fragments straight from global memory into registers (sk_chunks).  SK = 2: staged through the LDS tile.
//   template parameters read:  SK, KS, MB, NB (never PAIR, EX or SP: the body's static_asserts; 4 waves, tid = the body's)
//   names of the body read:    A, ex, ISP, cout0, kh, l31, wave, tid, NT, valid, voff, ox0, oy0, oz0, smem16 (SK = 2)
//   writes:                    acc; inv2 (the unscale factor the epilogue then takes instead of the main convolution's);
//                              SK = 2: the first buffer of smem16
//   barriers:                  SK = 1: none, no LDS access.  SK = 2: two per skip chunk; the first of them also waits for the
//                              last tap loop to be done with the tile.
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
