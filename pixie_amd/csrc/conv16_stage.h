// pixie_amd/csrc/conv16_stage.h -- FRAGMENT of conv3d_f16x3_body (conv16_body.h), included inside it after the weight pointers and
// before conv16_taps.h: the staging lambda  stage_chunk(c_base, buf, stid, nthr, s0, s1).  No include guard: included once.
// It brings the 16 input channels c_base .. c_base + 15 of the tile's halo'd voxels from global memory through the prologue (norm
// affine, LayerNorm affine, activation, zero padding after the activation, nearest x2, concat) into the LDS buffer `buf`: slots
// s0 + stid + k nthr of [s0, s1), as fp16 hi/lo planes (EX: fp32 planes, all of [0, CS), s0 / s1 unused).
//   template parameters read:  EX, SP, KS, MB, NB (the last three only for BUF: which instantiations load through buffer resources)
//   names of the body read:    A, lane, lx0, ly0, lz0, ISP, sx
//   writes:                    LDS at buf, nothing else; no name of the body
//   barriers:                  none inside.  The caller puts a barrier between the last read of `buf` and this call, and one between
//                              this call and the first read.  Called by whole waves with wave-uniform arguments but stid (the 32
//                              prologue constants travel through v_readlane).
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
        // Addresses, as in the register-fed skip (conv16_skip.h): raw buffer loads over the chunk's first channel plane, the plane as the scalar
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
