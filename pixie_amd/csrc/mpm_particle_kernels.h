// pixie_amd/csrc/mpm_particle_kernels.h -- MPM device code: particle modifiers, the separable transfer cores and the fused block kernel.
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// ------------------------------------------------------------------ particle modifiers
// apply_force (mpm_solver_warp.py:1015-1027), modify_particle_v_before_p2g (:1061-1073, :1137-1179)
__device__ __forceinline__ void apply_pmod(const PModDev& m, int caller_idx, float time, float dt, float mass,
                                           const float x[3], float v[3]) {
    if (!(time >= m.start && time < m.end)) return;
    if (m.mask[caller_idx] != 1) return;
    if (m.type == PIXIE_PM_IMPULSE) {
        for (int d = 0; d < 3; ++d) v[d] = v[d] + (m.force[d] / mass) * dt;
    } else if (m.type == PIXIE_PM_TRANSLATION) {
        for (int d = 0; d < 3; ++d) v[d] = m.velocity[d];
    } else {
        const float o[3] = {x[0] - m.point[0], x[1] - m.point[1], x[2] - m.point[2]};
        const float dn = o[0] * m.normal[0] + o[1] * m.normal[1] + o[2] * m.normal[2];
        const float hx = o[0] - dn * m.normal[0], hy = o[1] - dn * m.normal[1], hz = o[2] - dn * m.normal[2];
        const float hd = sqrtf(hx * hx + hy * hy + hz * hz);
        const float cosine = (o[0] * m.h1[0] + o[1] * m.h1[1] + o[2] * m.h1[2]) / hd;
        float theta = acosf(cosine);
        if (!((o[0] * m.h2[0] + o[1] * m.h2[1] + o[2] * m.h2[2]) > 0.0f)) theta = -theta;
        const float a1 = -hd * sinf(theta) * m.rot_scale;
        const float a2 = hd * cosf(theta) * m.rot_scale;
        for (int d = 0; d < 3; ++d) v[d] = a1 * m.h1[d] + a2 * m.h2[d] + m.trans_scale * m.normal[d];
    }
}

__device__ __forceinline__ bool stencil_inside(const Stencil& st, int ng) {
    bool ok = true;
    for (int d = 0; d < 3; ++d) ok = ok && (st.base[d] >= 0) && (st.base[d] + 2 < ng);
    return ok;
}

// ------------------------------------------------------------------ separable transfer cores
// The 27-node sums of g2p (mpm_utils.py:436-455) and p2g_apic_with_stress (:360-393) are tensor products of
// 1-D quadratic B-spline weights, so they are evaluated axis by axis (z innermost): 9 FMAs per node
// instead of ~28.  This only re-associates the reference's fp32 sums.
struct Weights1D {
    float w[3], dw[3], wd[3];  // weight, derivative (cell units), weight * (offset - fx)
};
__device__ __forceinline__ void weights_1d(const Stencil& st, int d, Weights1D& o) {
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        o.w[i] = st.w[d][i];
        o.dw[i] = st.dw[d][i];
        o.wd[i] = st.w[d][i] * ((float)i - st.fx[d]);
    }
}

// v = sum w g;  B_ab = sum w g_a dpos_b (cell units);  G_ab = sum g_a dweight_b (cell units)
// Two contractions of every node value g_a(i,j,k) carry all 21 sums (6 FMAs per node instead of 9; 288 VALU instructions per
// particle instead of 441 -- round 4, the kernel is VALU-issue bound):
//   s_a(i,j) = sum_k wz_k g_a       -> the x- and y-derivative columns:  ss_a(i) = sum_j wy_j s_a,  t_a(j) = sum_i wx_i s_a
//   h_a(k)   = sum_ij wx_i wy_j g_a -> v and the z-derivative column
//   v_a = sum_k wz_k h_a(k);   G_a0 = sum_i dwx_i ss_a(i),  G_a1 = sum_j dwy_j t_a(j),  G_a2 = sum_k dwz_k h_a(k);   B likewise with wd.
// SCHED: keep the loads of one x-slab from being hoisted over the previous slab's arithmetic (the 5-waves-per-SIMD register
// budget needs it; the wide variant for small scenes, F_WIDE, lets the compiler overlap everything).
template <bool SCHED, class Fetch>
__device__ __forceinline__ void g2p_gather(const Stencil& st, Fetch fetch, float nv[3], Mat3& B, Mat3& G) {
    Weights1D wx, wy, wz;
    weights_1d(st, 0, wx); weights_1d(st, 1, wy); weights_1d(st, 2, wz);
    float h[3][3], t[3][3], g0[3], b0[3];   // h[k][a], t[j][a]
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        g0[a] = 0.0f; b0[a] = 0.0f;
#pragma unroll
        for (int o = 0; o < 3; ++o) { h[o][a] = 0.0f; t[o][a] = 0.0f; }
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float ss[3] = {0, 0, 0};
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float wij = wx.w[i] * wy.w[j];
            float s[3] = {0, 0, 0};
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float g[3];
                fetch(i, j, k, g);
#pragma unroll
                for (int a = 0; a < 3; ++a) {
                    s[a] = fmaf(wz.w[k], g[a], s[a]);
                    h[k][a] = fmaf(wij, g[a], h[k][a]);
                }
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) {
                ss[a] = fmaf(wy.w[j], s[a], ss[a]);
                t[j][a] = fmaf(wx.w[i], s[a], t[j][a]);
            }
        }
#pragma unroll
        for (int a = 0; a < 3; ++a) {
            g0[a] = fmaf(wx.dw[i], ss[a], g0[a]);
            b0[a] = fmaf(wx.wd[i], ss[a], b0[a]);
        }
        if (SCHED) __builtin_amdgcn_sched_barrier(0);  // keep the 27 loads of the next x-slab from being hoisted over this one
    }
#pragma unroll
    for (int a = 0; a < 3; ++a) {
        nv[a] = fmaf(wz.w[2], h[2][a], fmaf(wz.w[1], h[1][a], wz.w[0] * h[0][a]));
        G.m[3 * a + 0] = g0[a];
        B.m[3 * a + 0] = b0[a];
        G.m[3 * a + 1] = fmaf(wy.dw[2], t[2][a], fmaf(wy.dw[1], t[1][a], wy.dw[0] * t[0][a]));
        B.m[3 * a + 1] = fmaf(wy.wd[2], t[2][a], fmaf(wy.wd[1], t[1][a], wy.wd[0] * t[0][a]));
        G.m[3 * a + 2] = fmaf(wz.dw[2], h[2][a], fmaf(wz.dw[1], h[1][a], wz.dw[0] * h[0][a]));
        B.m[3 * a + 2] = fmaf(wz.wd[2], h[2][a], fmaf(wz.wd[1], h[1][a], wz.wd[0] * h[0][a]));
    }
}

// momentum_a(i,j,k) = w (mv_a + A_a . dpos) + T_a . gradw,  mass(i,j,k) = w m   with A = m C' dx (dpos in cell
// units) and T = -dt vol inv_dx tau (gradw in cell units).  Grouped by axis (wd = w * offset, dw = dw/dx in cell units):
//   momentum_a = wz_k [ wy_j E_a(i) + wx_i U_a(j) ] + wx_i wy_j S_a(k)
//   E_a(i) = wx_i mv_a + A_a0 wdx_i + T_a0 dwx_i,   U_a(j) = A_a1 wdy_j + T_a1 dwy_j,   S_a(k) = A_a2 wdz_k + T_a2 dwz_k
// U and S do not depend on the other axes and are formed once per particle: 7 VALU instructions per node, 8 per (i, j)
// pair, 9 per x-slab, 36 once -- 324 per particle (round 3: 486; the block kernel is VALU-issue bound).
template <bool SCHED, class Emit>
__device__ __forceinline__ void p2g_scatter(const Stencil& st, const float mv[3], const Mat3& A, const Mat3& T, float mass, Emit emit) {
    Weights1D wx, wy, wz;
    weights_1d(st, 0, wx); weights_1d(st, 1, wy); weights_1d(st, 2, wz);
    float U[3][3], S[3][3];   // [component][offset]
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int o = 0; o < 3; ++o) {
            U[a][o] = fmaf(A.m[3 * a + 1], wy.wd[o], T.m[3 * a + 1] * wy.dw[o]);
            S[a][o] = fmaf(A.m[3 * a + 2], wz.wd[o], T.m[3 * a + 2] * wz.dw[o]);
        }
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        float E[3];
#pragma unroll
        for (int a = 0; a < 3; ++a) E[a] = fmaf(A.m[3 * a + 0], wx.wd[i], fmaf(T.m[3 * a + 0], wx.dw[i], wx.w[i] * mv[a]));
#pragma unroll
        for (int j = 0; j < 3; ++j) {
            const float wij = wx.w[i] * wy.w[j];
            float P[3];
#pragma unroll
            for (int a = 0; a < 3; ++a) P[a] = fmaf(E[a], wy.w[j], wx.w[i] * U[a][j]);
            const float M = wij * mass;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                float mom[3];
#pragma unroll
                for (int a = 0; a < 3; ++a) mom[a] = fmaf(wz.w[k], P[a], wij * S[a][k]);
                emit(i, j, k, mom, wz.w[k] * M);
            }
        }
        if (SCHED) __builtin_amdgcn_sched_barrier(0);
    }
}

// ---- slow path: a particle whose stencil lies outside its workgroup's tile talks to HBM directly.  Rare
// (stale binning only), so it is kept out of line and rolled to stay out of the fast path's register budget.
__device__ __noinline__ void g2p_gather_global(const float4* __restrict__ gout, int ng, Stencil st, float* nv9 /* nv[3], B[9], G[9] */) {
    float nv[3] = {0, 0, 0}, B[9], G[9];
    for (int q = 0; q < 9; ++q) { B[q] = 0.0f; G[q] = 0.0f; }
    const size_t r0 = ((size_t)st.base[0] * ng + st.base[1]) * ng + st.base[2];
#pragma unroll 1
    for (int t = 0; t < 27; ++t) {
        const int i = t / 9, j = (t / 3) % 3, k = t % 3;
        const float4 q = gout[r0 + ((size_t)i * ng + j) * ng + k];
        const float g[3] = {q.x, q.y, q.z};
        const float w = st.w[0][i] * st.w[1][j] * st.w[2][k];
        const float gw[3] = {st.dw[0][i] * st.w[1][j] * st.w[2][k], st.w[0][i] * st.dw[1][j] * st.w[2][k],
                             st.w[0][i] * st.w[1][j] * st.dw[2][k]};
        const float dp[3] = {(float)i - st.fx[0], (float)j - st.fx[1], (float)k - st.fx[2]};
        for (int a = 0; a < 3; ++a) {
            nv[a] += w * g[a];
            for (int b = 0; b < 3; ++b) {
                B[3 * a + b] += w * g[a] * dp[b];
                G[3 * a + b] += g[a] * gw[b];
            }
        }
    }
    for (int a = 0; a < 3; ++a) nv9[a] = nv[a];
    for (int q = 0; q < 9; ++q) { nv9[3 + q] = B[q]; nv9[12 + q] = G[q]; }
}

__device__ __noinline__ bool p2g_scatter_global(float4* gin, int* blk_flags, int nbk, int ng, Stencil st,
                                                const float* mvAT /* mv[3], A[9], T[9] */, float mass) {
    const size_t r0 = ((size_t)st.base[0] * ng + st.base[1]) * ng + st.base[2];
    // the 3x3x3 stencil touches at most 2 blocks per axis: tell the grid kernel they hold gin contributions.  The grid
    // kernel only visits ACTIVE blocks (particles within one block at the last re-binning); a particle that has left
    // all of them drifted >= 3 cells since then although the re-binning cadence is set to keep the drift below half a
    // cell (rebin()) -- it is dropped and counted, like a particle that leaves the grid.
    bool reachable = true;
    for (int c = 0; c < 8; ++c) {
        const int bx = (st.base[0] + 2 * (c >> 2)) / kBS, by = (st.base[1] + 2 * ((c >> 1) & 1)) / kBS, bz = (st.base[2] + 2 * (c & 1)) / kBS;
        reachable = reachable && (atomicOr(&blk_flags[(bx * nbk + by) * nbk + bz], 2) & 1);
    }
    if (!reachable) return false;
#pragma unroll 1
    for (int t = 0; t < 27; ++t) {
        const int i = t / 9, j = (t / 3) % 3, k = t % 3;
        const float w = st.w[0][i] * st.w[1][j] * st.w[2][k];
        const float gw[3] = {st.dw[0][i] * st.w[1][j] * st.w[2][k], st.w[0][i] * st.dw[1][j] * st.w[2][k],
                             st.w[0][i] * st.w[1][j] * st.dw[2][k]};
        const float dp[3] = {(float)i - st.fx[0], (float)j - st.fx[1], (float)k - st.fx[2]};
        float* cell = reinterpret_cast<float*>(gin + r0 + ((size_t)i * ng + j) * ng + k);
        for (int a = 0; a < 3; ++a) {
            const float* A = mvAT + 3 + 3 * a;
            const float* T = mvAT + 12 + 3 * a;
            const float mom = w * (mvAT[a] + A[0] * dp[0] + A[1] * dp[1] + A[2] * dp[2]) + T[0] * gw[0] + T[1] * gw[1] + T[2] * gw[2];
            unsafeAtomicAdd(cell + a, mom);
        }
        unsafeAtomicAdd(cell + 3, w * mass);
    }
    return true;
}

// ------------------------------------------------------------------ fused block kernel
// G2P part: g2p (mpm_utils.py:412-463).  P2G part: pre-P2G modifiers, compute_stress_from_F_trial
// (:467-526) and p2g_apic_with_stress (:338-394).  `sp.time` is the time of the substep whose P2G runs.
//
// The scatter accumulates in LDS with 64-bit INTEGER atomics: ds_add_f32 retires ~1 lane per 3 cycles on gfx950
// (193 cycles per wave-instruction, measured: scripts/microbench/lds_atomics.hip), ds_add_u64 is 11x faster.  Each
// workgroup therefore (1) computes every particle's scatter inputs, (2) takes the workgroup maximum of a bound on
// their contributions, (3) scales by the power of two that puts that bound just below 2^42 and adds round-to-nearest
// integers (|sum of 256| < 2^50; see to_fixed).  The LSB is 2^-42 of the largest contribution in the tile, i.e. the tile
// sums are exact to ~2e-13 -- tighter than any fp32 summation order -- and since integer adds commute they are bit-reproducible.
// (A 32-bit variant -- LSB 2^-21 -- was measured first: low-mass free-surface nodes lost up to 10 % of their velocity.)
struct ScatterIn {
    float x[3];     // position after the G2P update (where the P2G stencil is taken)
    float mv[3];    // mass * v
    Mat3 A;         // mass * C' * dx
    Mat3 T;         // -dt * vol * inv_dx * tau
    float mass;
    bool active;    // contributes to P2G
};

// what a particle needs from HBM before it can start: issued BEFORE the tile load + barrier so that the two latencies overlap
struct Preload {
    float x[3];
    Mat3 F;          // fused kernel: F of the previous substep (G2P input); P2G-only kernel: unused
    float mass, vol, mu, lam;
    int material, selection;
};
template <bool DO_G2P, bool DO_P2G>
__device__ __forceinline__ void preload_particle(const MpmPtrs& S, int p, Preload& L) {
    const int n = S.n;
    L.selection = S.selection[p];
#pragma unroll
    for (int d = 0; d < 3; ++d) L.x[d] = S.x[d * n + p];
    if (DO_G2P) {
#pragma unroll
        for (int i = 0; i < 9; ++i) L.F.m[i] = S.F[i * n + p];
    }
    if (DO_P2G) {
        L.mass = S.mass[p]; L.vol = S.vol[p]; L.mu = S.mu[p]; L.lam = S.lam[p]; L.material = S.material[p];
    }
}

// What a caller reads from a particle that has just been frozen outside the grid: zero velocity and APIC matrix, and its last
// deformation gradient as F_trial.  (The fused kernel keeps v, C and F_trial of the particles that take part in registers, and a
// re-binning does not move those rows for them -- bin_permute_kernel -- so the rows of a particle that drops out are written here.)
// (inlined, a rolled loop of plain stores: an out-of-line function taking the kernel's parameter struct by reference copies it to
// scratch -- 404 -> 740 bytes per lane, beyond the cliff of profiles/r6e_scratch_regression.txt)
__device__ __forceinline__ void freeze_particle_state(const MpmPtrs& S, int p, const Mat3& F) {
    const int n = S.n;
#pragma unroll
    for (int d = 0; d < 3; ++d) S.v[d * n + p] = 0.0f;
#pragma unroll
    for (int i = 0; i < 9; ++i) { S.C[i * n + p] = 0.0f; S.Ft[i * n + p] = F.m[i]; }
}

template <bool DO_G2P, bool DO_P2G, bool SCHED>
__device__ __forceinline__ void particle_phase1(const MpmPtrs& S, const StepParams& sp, const PModSet& pms, int p, int ox, int oy,
                                                int oz, const float4* tv, const Preload& L, ScatterIn& out) {
    out.active = false;
    if (L.selection != 0) return;
    const int n = S.n;
    float x[3], v[3];
    Mat3 C, Ft;
#pragma unroll
    for (int d = 0; d < 3; ++d) x[d] = L.x[d];

    if (DO_G2P) {
        const Stencil st = make_stencil(x[0], x[1], x[2], S.inv_dx);
        if (!stencil_inside(st, S.ng)) {
            atomicAdd(S.oob, 1ull);
            S.selection[p] = 2;   // left the grid: frozen from now on and counted once (UB in the reference)
            freeze_particle_state(S, p, L.F);
            return;
        }
        const Mat3& Fold = L.F;
        float nv[3];
        Mat3 B, G;
        const int lx = st.base[0] - ox, ly = st.base[1] - oy, lz = st.base[2] - oz;
        if ((unsigned)lx <= (unsigned)(kTS - 3) && (unsigned)ly <= (unsigned)(kTS - 3) && (unsigned)lz <= (unsigned)(kTS - 3)) {
            const int b0 = (lx * kTS + ly) * kTS + lz;
            g2p_gather<SCHED>(st, [&](int i, int j, int k, float g[3]) {
                // One ds_read_b128 per node.  The .w lane is dead, but a 16-byte LDS read costs 4 LDS cycles per wave against
                // 8 for the 12-byte ds_read_b96 the compiler would narrow it to (MI355X_MICROARCH.md, LDS table), and LDS
                // and VALU time add up in this kernel (80.7 -> 78.4 us per launch at 1 M particles): keep the lane alive.
                const float4 q = tv[b0 + (i * kTS + j) * kTS + k];
                asm volatile("" :: "v"(q.w));
                g[0] = q.x; g[1] = q.y; g[2] = q.z;
            }, nv, B, G);
        } else {
            atomicAdd(S.oob + 1, 1ull);
            float acc[21];
            g2p_gather_global(S.gout, S.ng, st, acc);
#pragma unroll
            for (int a = 0; a < 3; ++a) nv[a] = acc[a];
#pragma unroll
            for (int q = 0; q < 9; ++q) { B.m[q] = acc[3 + q]; G.m[q] = acc[12 + q]; }
        }
        Mat3 Amat;
        const float sdt = sp.dt * S.inv_dx;
#pragma unroll
        for (int i = 0; i < 9; ++i) Amat.m[i] = ((i % 4 == 0) ? 1.0f : 0.0f) + G.m[i] * sdt;
        Ft = mat_mul(Amat, Fold);
        const float sc = 4.0f * S.inv_dx;
#pragma unroll
        for (int i = 0; i < 9; ++i) C.m[i] = B.m[i] * sc;
        // x += dt v in float32 (mpm_utils.py:447) drops whatever of dt v lies below ulp(x)/2 = 6e-8 at x ~ 1: in a quiet scene
        // (dt v ~ 1e-7) most of the motion, systematically -- the reference's own float32 behaviour, and the default here.
        // "compensated_x" keeps what was dropped in xlo and feeds it into the next increment (Kahan): x is then the float32
        // ROUNDING of the accumulated position instead of a sum of rounded increments (3 more words per particle each way).
#pragma unroll
        for (int d = 0; d < 3; ++d) {
            v[d] = nv[d];
            if (sp.comp_x) {
                const float y = sp.dt * nv[d] + S.xlo[d * n + p];
                const float t = x[d] + y;
                S.xlo[d * n + p] = y - (t - x[d]);
                x[d] = t;
            } else {
                x[d] = x[d] + sp.dt * nv[d];
            }
            S.x[d * n + p] = x[d];
        }
        if (!DO_P2G) {  // the state a caller can observe: x, v, C, F_trial
#pragma unroll
            for (int d = 0; d < 3; ++d) S.v[d * n + p] = v[d];
#pragma unroll
            for (int i = 0; i < 9; ++i) {
                S.C[i * n + p] = C.m[i];
                S.Ft[i * n + p] = Ft.m[i];
            }
            return;
        }
    } else {
#pragma unroll
        for (int d = 0; d < 3; ++d) v[d] = S.v[d * n + p];
#pragma unroll
        for (int i = 0; i < 9; ++i) {
            C.m[i] = S.C[i * n + p];
            Ft.m[i] = S.Ft[i * n + p];
        }
    }

    if (DO_P2G) {
        const float mass = L.mass;
        if (pms.n > 0) {
            const float v_before[3] = {v[0], v[1], v[2]};
            const int ci = S.perm[p];
            for (int k = 0; k < pms.n; ++k) apply_pmod(pms.pm[k], ci, sp.time, sp.dt, mass, x, v);
            if (!DO_G2P && (v[0] != v_before[0] || v[1] != v_before[1] || v[2] != v_before[2]))
                for (int d = 0; d < 3; ++d) S.v[d * n + p] = v[d];
        }
        const int material = L.material;
        float mu = L.mu, lam = L.lam;
        float ys = (material == 1 || material == 3 || material == 5) ? S.ys[p] : 0.0f;
        const float bulk = (material == 6) ? S.bulk[p] : 0.0f;
        const float mu0 = mu, lam0 = lam, ys0 = ys;
        Mat3 F, tau;
        return_map_and_stress(material, Ft, mu, lam, bulk, ys, sp.ms, sp.dt, F, tau);
#pragma unroll
        for (int i = 0; i < 9; ++i) S.F[i * n + p] = F.m[i];
        if (ys != ys0) S.ys[p] = ys;
        if (mu != mu0) S.mu[p] = mu;
        if (lam != lam0) S.lam[p] = lam;

        // C' = (1-r) C + r/2 (C - C^T);  r < -0.001 => PIC (mpm_utils.py:372-379)
#pragma unroll
        for (int a = 0; a < 3; ++a)
#pragma unroll
            for (int b = 0; b < 3; ++b) {
                float c = (1.0f - sp.rpic) * C.m[3 * a + b] + sp.rpic * 0.5f * (C.m[3 * a + b] - C.m[3 * b + a]);
                if (sp.rpic < -0.001f) c = 0.0f;
                out.A.m[3 * a + b] = mass * c * S.dx;  // dpos = (ijk - fx) * dx
            }
        const float ks = -sp.dt * L.vol * S.inv_dx;  // dt * (-vol * tau * dweight), dweight = dw*w*w*inv_dx
#pragma unroll
        for (int i = 0; i < 9; ++i) out.T.m[i] = ks * tau.m[i];
#pragma unroll
        for (int d = 0; d < 3; ++d) { out.mv[d] = mass * v[d]; out.x[d] = x[d]; }
        out.mass = mass;
        out.active = true;
    }
}

// ---- fixed-point accumulation of the scatter ---------------------------------------------------------------------------
// EXACT mode (set_scalar "scatter_bits" 64): 64-bit fixed point through the double-precision adder: the mantissa field of (x + 1.5 * 2^52) is
// 2^51 + round(x) for |x| < 2^51, so ds_add_u64 of the raw bit patterns accumulates sum(round(x_i)) modulo 2^51 in the low
// 51 bits whatever happens above them (the N copies of the exponent and of the 2^51 offset only carry upwards).  With every
// contribution scaled below 2^42 and at most 256 of them per node the sum stays below 2^50 and is recovered by
// sign-extending bit 50: two instructions per contribution (v_cvt_f64_f32, v_add_f64), exact integer accumulation,
// order-independent.
// PACKED mode (F_PACK32, the default; "scatter_bits" 32): two 32-bit two's-complement integers per ds_add_u64 -- (m*v.x, m*v.y)
// and (m, m*v.z) -- so a node costs 2 LDS atomics instead of 4 and 6 plain VALU instructions instead of 8 double-rate ones.
// The contributions are scaled so that the sum of the particles' bounds is below 2^30 (see the scales in the kernel) and
// rounded to nearest by v_cvt_rpi_i32_f32; the
// pair word is low + (high << 32) in 64-bit arithmetic, i.e. the high dword carries `high + (low >> 31)`, and the decode
// undoes exactly that, so the two sums are exact integers and order-independent like the 64-bit ones.  What changes is the
// quantum: 2^-30 of the SUM of the contribution bounds of the tile's particles instead of 2^-42 of their maximum -- the
// order of the fp32 atomics of the reference (2^-24 of each partial sum) for nodes that carry mass, but a node whose whole
// mass is below ~1e-7 of a particle's (stencil corners at a free surface) is quantised visibly: see HISTORY.md 3.5 and
// tests/test_mpm_hip.py::test_packed_scatter_parity.
constexpr double kMagicD = 6755399441055744.0;            // 1.5 * 2^52

// power of two s with bound * s in [2^top, 2^(top+1))  (1 when the bound is zero / not finite)
__device__ __forceinline__ float scale_for(float bound, int top) {
    const unsigned bits = __float_as_uint(bound);
    const int eb = (int)((bits >> 23) & 0xffu) - 127;
    if (!(bound > 0.0f) || eb > 120) return 1.0f;
    int e = top - eb;
    e = e > 120 ? 120 : (e < -80 ? -80 : e);
    return __uint_as_float((unsigned)(e + 127) << 23);
}
// 1 / s for s = 2^e, exactly, without a division (|e| <= 120: scale_for)
__device__ __forceinline__ float pow2_reciprocal(float s) {
    return __uint_as_float(0x7f000000u - __float_as_uint(s));
}
__device__ __forceinline__ unsigned long long to_fixed(float scaled) {
    return (unsigned long long)__double_as_longlong((double)scaled + kMagicD);
}
// low 51 bits, sign-extended, as a float: flipping bit 50 turns the field into (sum + 2^50) >= 0, which is dropped into the
// mantissa of 2^52 and the two offsets subtracted again -- exact (|sum| < 2^50), and no 64-bit integer conversion
__device__ __forceinline__ float from_fixed(unsigned long long v, float inv_scale) {
    const unsigned hi = (((unsigned)(v >> 32) & 0x7ffffu) ^ 0x40000u) | 0x43300000u;
    const double d = __hiloint2double((int)hi, (int)(unsigned)v) - 5629499534213120.0;   // 2^52 + 2^50
    return (float)(d * (double)inv_scale);
}
__device__ __forceinline__ int round_to_int(float x) {   // floor(x + 0.5): one instruction (CDNA keeps GCN's v_cvt_rpi)
    int r;
    asm("v_cvt_rpi_i32_f32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ int round_to_int_neg(float x) {   // floor(-x + 0.5): the negation rides in the VOP3 source modifier
    int r;
    asm("v_cvt_rpi_i32_f32_e64 %0, -%1" : "=v"(r) : "v"(x));
    return r;
}
__device__ __forceinline__ unsigned long long pack_pair(int low, int high) {
    return (unsigned long long)(unsigned)low | ((unsigned long long)(unsigned)(high + (low >> 31)) << 32);
}
__device__ __forceinline__ void unpack_pair(unsigned long long w, int& low, int& high) {
    low = (int)(unsigned)w;
    high = (int)(unsigned)(w >> 32) - (low >> 31);
}

// Maximum of a non-negative float over the wave, in the DPP network (no LDS round trips: __shfl_xor is ds_bpermute, six
// dependent ~60-cycle LDS operations per value).  Non-negative floats order like their bit patterns, so the maximum is
// taken on integers (no NaN canonicalisation instructions; a NaN bound comes out as the maximum, which scale_for maps to 1).
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ unsigned dpp_umax(unsigned v) {
    // lanes the pattern does not feed (masked rows) read their own value: old = v, bound_ctrl off
    const unsigned o = (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, ROW_MASK, 0xf, false);
    return max(v, o);
}
// Sum over the wave in the same network (fixed tree: reproducible).  Lanes a masked row pattern does not feed add 0.
template <int CTRL, int ROW_MASK>
__device__ __forceinline__ float dpp_add(float v) {
    const int o = __builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, ROW_MASK, 0xf, false);
    return v + __int_as_float(o);
}
__device__ __forceinline__ float wave_sum(float v) {
    v = dpp_add<0xB1, 0xf>(v);
    v = dpp_add<0x4E, 0xf>(v);
    v = dpp_add<0x141, 0xf>(v);
    v = dpp_add<0x140, 0xf>(v);     // every lane of a row of 16 holds the row sum
    v = dpp_add<0x142, 0xa>(v);     // rows 1, 3 += rows 0, 2
    v = dpp_add<0x143, 0xc>(v);     // rows 2, 3 += row 1 (= rows 0 + 1): lane 63 holds the wave sum
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), 63));
}
__device__ __forceinline__ float wave_max_nonneg(float x) {
    unsigned v = __float_as_uint(x);
    v = dpp_umax<0xB1, 0xf>(v);     // quad_perm [1,0,3,2]
    v = dpp_umax<0x4E, 0xf>(v);     // quad_perm [2,3,0,1]
    v = dpp_umax<0x141, 0xf>(v);    // row_half_mirror
    v = dpp_umax<0x140, 0xf>(v);    // row_mirror: every lane of a row of 16 holds the row maximum
    v = dpp_umax<0x142, 0xa>(v);    // row_bcast:15 into rows 1 and 3
    v = dpp_umax<0x143, 0xc>(v);    // row_bcast:31 into rows 2 and 3: lane 63 holds the wave maximum
    return __uint_as_float((unsigned)__builtin_amdgcn_readlane((int)v, 63));
}

// Phase trace (pixie_mpm_set_scalar "trace" 1; read back with pixie::mpm_trace_read, not part of the C ABI): per work item 8
// 100 MHz timestamps -- start, tile staged, particles updated (G2P + stress), scales known, scatter done, tile published.
// The trace buffer, the F_TRACE instantiation and every diagnostic entry point exist only in the -DPIXIE_DIAG build
// (libpixie_hip_diag.so: tests and profilers); the production library carries none of it.
#ifdef PIXIE_DIAG
constexpr int kMpmTraceItems = 32768;
__device__ unsigned long long g_mpm_trace[kMpmTraceItems * 8];
#define PX_MPM_STAMP(i) do { if ((FL & F_TRACE) && (sp.trace & 1) && tid == 0 && blockIdx.x < (unsigned)kMpmTraceItems) g_mpm_trace[blockIdx.x * 8 + (i)] = wall_clock64(); } while (0)
#else
#define PX_MPM_STAMP(i) do { } while (0)
#endif

// kernel variants (FL)
constexpr int F_TRACE = 1;    // phase stamps + the ablation switches of StepParams.trace (timing studies only)
constexpr int F_PACK32 = 2;   // packed 32-bit scatter (above)
constexpr int F_WIDE = 8;     // no scheduling barriers: for scenes too small to fill the chip, where latency, not issue, binds

// OCC = waves per SIMD the register allocation is held to (launch_bounds).  Built without the SLP vectoriser (see
// pixie_amd/build.py) the kernel needs 96 VGPRs -> 5 waves per SIMD with no spills (with it: 168 VGPRs, 3 waves, and
// 20 % slower); 6 -> 80 VGPRs with ~20 spilled dwords (measured slower: 86 vs 81 us at 1 M particles).  Chosen at run
// time (set_scalar "occupancy"), same arithmetic.
template <bool DO_G2P, bool DO_P2G, int OCC, int FL>
__global__ __launch_bounds__(kWG, OCC) void mpm_block_kernel(MpmPtrs S, StepParams sp, PModSet pms) {
    constexpr bool PACK = (FL & F_PACK32) != 0;
    constexpr bool TRACE = (FL & F_TRACE) != 0;
    constexpr bool SCHED = (FL & F_WIDE) == 0;
    __shared__ float4 tv[kTN];    // grid velocities of the tile (G2P source)
    __shared__ unsigned long long ta[PACK ? 2 : 4][kTN];  // (m*v.xyz, m) of this work item as scaled integers (P2G target)
    __shared__ float s_red[2][kWG / 64];
    // Workgroups are dealt to the 8 XCDs round-robin (workgroup b runs on XCD b % 8) and each XCD has its own L2.  The work list is in
    // block order, so with sp.xcd_order every XCD takes a CONTIGUOUS eighth of it: neighbouring blocks -- whose 8^3 tiles of gout
    // overlap eightfold -- then share their staging reads in that XCD's L2 instead of fetching them once per XCD
    // (set_scalar "xcd_order", on by default: -2.6 % per substep at 1 M and 100 k, bit-identical results; the tile a work item
    // publishes is addressed by the item, not by the workgroup).
    int item = (int)blockIdx.x;
    if (sp.xcd_order) {
        const int per = (int)gridDim.x >> 3;
        if (item < (per << 3)) item = (item & 7) * per + (item >> 3);      // (the last n % 8 items keep their place)
    }
#include "mpm_block_body.h"
}

}  // namespace pixie
