// pixie_amd/csrc/mpm_block_body.h -- the body of the fused MPM block kernel: ONE work item (G2P, modifiers, return map + stress,
// P2G into the item's LDS tile, publish).  Included INSIDE the two kernels that run it -- mpm_block_kernel (one scene, parameters
// as kernel arguments) and mpm_block_batch_kernel (several scenes, parameters from per-scene descriptors) -- after they have
// defined, in scope:
//   template parameters DO_G2P, DO_P2G, FL;  const MpmPtrs& / MpmPtrs S;  StepParams sp;  PModSet pms;
//   int item: the work item in S.items (which also addresses the tile it publishes).
// (Textual inclusion, not a __forceinline__ function: moved into a function, the same statements compile to a different register
// allocation of the solo kernel -- 87 -> 91 VGPRs, another scratch layout -- and the solo kernels must stay exactly as they are.)
// No include guard: included once per kernel.
    const int4 it = S.items[item];
    const int tid = threadIdx.x;
    const int nthr = blockDim.x;   // = the work-item capacity of the current binning (256; 128 on request)
    const int bz = it.x % S.nbk, by = (it.x / S.nbk) % S.nbk, bx = it.x / (S.nbk * S.nbk);
    const int ox = bx * kBS - 1, oy = by * kBS - 1, oz = bz * kBS - 1;
    const int ng = S.ng;
    PX_MPM_STAMP(0);
    Preload L;
    L.selection = 1;
    if (tid < it.z) preload_particle<DO_G2P, DO_P2G>(S, it.y + tid, L);   // in flight while the tile is staged
    for (int idx = tid; idx < kTN; idx += nthr) {
        if (DO_G2P) {
            const int gz = oz + (idx & (kTS - 1)), gy = oy + ((idx >> 3) & (kTS - 1)), gx = ox + (idx >> 6);
            float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((unsigned)gx < (unsigned)ng && (unsigned)gy < (unsigned)ng && (unsigned)gz < (unsigned)ng && !(TRACE && (sp.trace & 0x400)))
                g = S.gout[((size_t)gx * ng + gy) * ng + gz];
            tv[idx] = g;
        }
        if (DO_P2G) {
            ta[0][idx] = 0ull; ta[1][idx] = 0ull;
            if (!PACK) { ta[2][idx] = 0ull; ta[3][idx] = 0ull; }
        }
    }
    __syncthreads();
    PX_MPM_STAMP(1);

    // One chunk of <= 256 particles per work item.  Sharing one tile between more particles was measured both ways and
    // loses: (a) a workgroup looping over several 256-particle chunks (integer sums folded into an fp32 tile between
    // chunks) -- hipcc 7.2 keeps 176 VGPRs live across the loop (3 waves per SIMD instead of 5); (b) work items of 384 ...
    // 1024 threads -- 107 ... 132 us per launch at 1 M particles against 81 us for 256 (r2g): every barrier then waits
    // for the slowest of 6 ... 16 waves.  The per-item costs (staging, zeroing, publish) are the smaller evil.
    const int q = tid;
    ScatterIn in;
    in.active = false;
    if (q < it.z) particle_phase1<DO_G2P, DO_P2G, SCHED>(S, sp, pms, it.y + q, ox, oy, oz, tv, L, in);
    if (!DO_P2G) return;
    PX_MPM_STAMP(2);

    // ---- P2G: a particle whose stencil left the tile goes straight to HBM (fp32 atomics into gin) ----
    Stencil st;
    int b0 = -1;
    if (in.active) {
        st = make_stencil(in.x[0], in.x[1], in.x[2], S.inv_dx);
        if (!stencil_inside(st, ng)) {
            atomicAdd(S.oob, 1ull);
            S.selection[it.y + q] = 2;
            Mat3 Fnow;
#pragma unroll
            for (int i = 0; i < 9; ++i) Fnow.m[i] = S.F[i * S.n + it.y + q];     // (the return-mapped F this launch has just stored)
            freeze_particle_state(S, it.y + q, Fnow);
            in.active = false;
        } else {
            const int lx = st.base[0] - ox, ly = st.base[1] - oy, lz = st.base[2] - oz;
            if ((unsigned)lx <= (unsigned)(kTS - 3) && (unsigned)ly <= (unsigned)(kTS - 3) && (unsigned)lz <= (unsigned)(kTS - 3)) {
                b0 = (lx * kTS + ly) * kTS + lz;
            } else {
                atomicAdd(S.oob + 1, 1ull);
                float mvAT[21];
#pragma unroll
                for (int a = 0; a < 3; ++a) mvAT[a] = in.mv[a];
#pragma unroll
                for (int k = 0; k < 9; ++k) { mvAT[3 + k] = in.A.m[k]; mvAT[12 + k] = in.T.m[k]; }
                if (!p2g_scatter_global(S.gin, S.blk_flags, S.nbk, ng, st, mvAT, in.mass)) atomicAdd(S.oob + 2, 1ull);
                in.active = false;
            }
        }
    }
    // ---- workgroup bounds -> power-of-two scales ----
    // One contribution of a particle is  w (mv_a + A_a . d) + T_a . g  with  w <= 0.75^3, |d_b| <= 1.5, |g_b| <= 0.75^2 (the
    // B-spline weights and their derivatives in cell units), so  r_p = max_a [0.421875 (|mv_a| + 1.5 sum_b |A_ab|) +
    // 0.5625 sum_b |T_ab|]  bounds every contribution of particle p.
    //   exact mode: scale by the workgroup MAXIMUM of r_p to [2^41, 2^42): 256 contributions stay below 2^50.
    //   packed mode: scale by the workgroup SUM of r_p to [2^29, 2^30): |any node sum| <= sum_p r_p < 2^30 whatever the
    //     particle count, and the quantum is 2^-30 of the SUM instead of 2^-22 of 256 maxima -- typically 10-20x finer
    //     (the sum of ~180 bounds of which most are well below the largest).  Same for the masses.
    float bp = 0.0f, bm = 0.0f;
    if (TRACE && (sp.trace & 0x200)) { bp = PACK ? 256.0f : 1.0f; bm = PACK ? 0.256f : 1e-3f; }
    else {
        if (in.active) {
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                const float r = 0.421875f * (fabsf(in.mv[a]) + 1.5f * (fabsf(in.A.m[3 * a]) + fabsf(in.A.m[3 * a + 1]) + fabsf(in.A.m[3 * a + 2]))) +
                                0.5625f * (fabsf(in.T.m[3 * a]) + fabsf(in.T.m[3 * a + 1]) + fabsf(in.T.m[3 * a + 2]));
                bp = fmaxf(bp, r);
            }
            bm = 0.421875f * in.mass;
        }
        if (PACK) { bp = wave_sum(bp); bm = wave_sum(bm); }
        else { bp = wave_max_nonneg(bp); bm = wave_max_nonneg(bm); }
        if ((tid & 63) == 0) { s_red[0][tid >> 6] = bp; s_red[1][tid >> 6] = bm; }
        __syncthreads();
        bp = s_red[0][0]; bm = s_red[1][0];
        for (int w = 1; w < (nthr >> 6); ++w) {
            if (PACK) { bp += s_red[0][w]; bm += s_red[1][w]; }     // (fixed order: the scale is reproducible)
            else { bp = fmaxf(bp, s_red[0][w]); bm = fmaxf(bm, s_red[1][w]); }
        }
    }
    constexpr int kTop = PACK ? 29 : 41;
    const float sP = scale_for(bp, kTop), sM = scale_for(bm, kTop);
    PX_MPM_STAMP(3);

    if (in.active) {
#pragma unroll
        for (int a = 0; a < 3; ++a) in.mv[a] *= sP;
#pragma unroll
        for (int k = 0; k < 9; ++k) { in.A.m[k] *= sP; in.T.m[k] *= sP; }
        p2g_scatter<SCHED>(st, in.mv, in.A, in.T, in.mass * sM, [&](int i, int j, int k, const float mom[3], float m) {
            const int idx = b0 + (i * kTS + j) * kTS + k;
            if (TRACE && (sp.trace & 0x100)) { asm volatile("" :: "v"(mom[0]), "v"(mom[1]), "v"(mom[2]), "v"(m)); return; }
            if (PACK) {
                // v_cvt_rpi rounds exact ties UP, and ties are common (a contribution of magnitude 2^22 is a float with one
                // fractional bit): left alone that is a drift of ~0.2 quanta per contribution in +x, +y, +z -- measured as
                // 3e-3 of the total momentum over 500 substeps.  Neighbouring nodes therefore alternate: (i + j + k) even
                // adds round(x), odd SUBTRACTS round(-x), i.e. rounds ties down.  Unbiased, and still a pure function of
                // the particle's own data (deterministic, order-independent).
                if (((i + j + k) & 1) == 0) {
                    atomicAdd(&ta[0][idx], pack_pair(round_to_int(mom[0]), round_to_int(mom[1])));
                    // the mass is never negative: in the low half it needs no borrow correction
                    atomicAdd(&ta[1][idx], (unsigned long long)(unsigned)round_to_int(m) | ((unsigned long long)(unsigned)round_to_int(mom[2]) << 32));
                } else {
                    __hip_atomic_fetch_sub(&ta[0][idx], pack_pair(round_to_int_neg(mom[0]), round_to_int_neg(mom[1])), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    __hip_atomic_fetch_sub(&ta[1][idx], pack_pair(round_to_int_neg(m), round_to_int_neg(mom[2])), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
            } else {
                atomicAdd(&ta[0][idx], to_fixed(mom[0]));
                atomicAdd(&ta[1][idx], to_fixed(mom[1]));
                atomicAdd(&ta[2][idx], to_fixed(mom[2]));
                atomicAdd(&ta[3][idx], to_fixed(m));
            }
        });
    }
    // where this thread's nodes go in the staged tile: fetched now, consumed behind the barrier
    const unsigned lut = (nthr == kWG) ? S.staged_lut[tid] : 0u;
    __syncthreads();
    PX_MPM_STAMP(4);
    const float iP = pow2_reciprocal(sP), iM = pow2_reciprocal(sM);
    // ---- publish the tile: coalesced stores; the grid update sums the tiles that cover each node ----
    float4* dst = S.part + (size_t)item * kTN;
    if (!(TRACE && (sp.trace & 0x800)))
        for (int idx = tid; idx < kTN; idx += nthr) {
            float4 o;
            if (PACK) {
                int px, py, pm, pz;
                unpack_pair(ta[0][idx], px, py);
                const unsigned long long w1 = ta[1][idx];
                pm = (int)(unsigned)w1; pz = (int)(unsigned)(w1 >> 32);
                o = make_float4((float)px * iP, (float)py * iP, (float)pz * iP, (float)pm * iM);
            } else {
                o = make_float4(from_fixed(ta[0][idx], iP), from_fixed(ta[1][idx], iP), from_fixed(ta[2][idx], iP), from_fixed(ta[3][idx], iM));
            }
            // (staged_index is ~30 instructions of selects per node; with the usual 256-thread work items each thread's two
            // nodes are tid and tid + 256 and their staged positions come from a 1 KB table, two 16-bit halves of one word)
            const int si = (nthr == kWG) ? (int)((idx < kWG) ? (lut & 0xffffu) : (lut >> 16)) : staged_index(idx >> 6, (idx >> 3) & 7, idx & 7);
            // Typically 40-60 % of a tile's nodes received nothing (the drift margin planes, corners beyond every stencil): they
            // are neither stored nor -- by the mask -- read back.  Adding an all-zero float4 is a no-op, so the sums are unchanged.
            const bool nz = (o.x != 0.0f) | (o.y != 0.0f) | (o.z != 0.0f) | (o.w != 0.0f);
            if (S.sparse_tiles) {
                const unsigned long long live = __ballot(nz);     // lanes of a wave hold 64 consecutive nodes
                if ((tid & 63) == 0) S.tile_mask[(size_t)item * 8 + (idx >> 6)] = live;
                if (nz) dst[si] = o;
            } else {
                dst[si] = o;
            }
        }
    PX_MPM_STAMP(5);
#ifdef PIXIE_DIAG
    if (TRACE && (sp.trace & 1) && tid == 0 && blockIdx.x < (unsigned)kMpmTraceItems)   // where it ran: HW_ID | XCC_ID << 32
        g_mpm_trace[blockIdx.x * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
#endif
