// pixie_amd/csrc/mpm_grid_kernels.h -- MPM device code: the active-block grid kernel (normalise, gravity, damping, BCs).
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// ------------------------------------------------------------------ grid kernel
// grid_normalization_and_gravity (mpm_utils.py:398-409), add_damping_via_grid (:583-588) and the
// BC `collide` closures (mpm_solver_warp.py:785-840 surface, :874-897 cuboid, :917-974 bounding box)
// in one sweep; also re-zeroes (m*v, m) so the next P2G starts from a clean grid (zero_grid :295-300).
// (No FMA contraction in apply_bc / finish_node: whether `float(k) * dx - point` is fused decides on which side of a collider plane a
// node plane lies (tests: knife-edge scene), and hipcc's choice depends on the code around it.  Every operation rounded, as in the
// float32 oracle -- the same bits in whatever kernel these are inlined into.)
__device__ __forceinline__ void apply_bc(const BCDev& b, int ix, int iy, int iz, int ng, float dx, float time,
                                         float dt, float v[3]) {
#pragma clang fp contract(off)
    if (b.type == PIXIE_BC_SURFACE) {
        if (time >= b.start && time < b.end) {
            const float ox = (float)ix * dx - b.point[0], oy = (float)iy * dx - b.point[1], oz = (float)iz * dx - b.point[2];
            const float dp = ox * b.normal[0] + oy * b.normal[1] + oz * b.normal[2];
            if (dp < 0.0f) {
                if (b.surface_type == 11) {
                    if ((float)iz * dx < 0.4f || (float)iz * dx > 0.53f) {
                        v[0] = v[1] = v[2] = 0.0f;
                    } else {
                        v[0] = v[0] * 0.3f; v[1] = 0.0f; v[2] = v[2] * 0.3f;
                    }
                } else {
                    // sticky, and -- as in the reference (:821-840) -- slip/friction too: the projected
                    // velocity is computed there but the store is zero.
                    v[0] = v[1] = v[2] = 0.0f;
                }
            }
        }
    } else if (b.type == PIXIE_BC_CUBOID) {
        if (time >= b.start && time < b.end) {
            const float ox = (float)ix * dx - b.point[0], oy = (float)iy * dx - b.point[1], oz = (float)iz * dx - b.point[2];
            if (fabsf(ox) < b.size[0] && fabsf(oy) < b.size[1] && fabsf(oz) < b.size[2]) {
                v[0] = b.velocity[0]; v[1] = b.velocity[1]; v[2] = b.velocity[2];
            }
        } else if (b.reset == 1) {
            if (time < b.end + 15.0f * dt) v[0] = v[1] = v[2] = 0.0f;
        }
    } else {
        const int padding = 3;
        if (time >= b.start && time < b.end) {
            if (ix < padding && v[0] < 0.0f) v[0] = 0.0f;
            if (ix >= ng - padding && v[0] > 0.0f) v[0] = 0.0f;
            if (iy < padding && v[1] < 0.0f) v[1] = 0.0f;
            if (iy >= ng - padding && v[1] > 0.0f) v[1] = 0.0f;
            if (iz < padding && v[2] < 0.0f) v[2] = 0.0f;
            if (iz >= ng - padding && v[2] > 0.0f) v[2] = 0.0f;
        }
    }
}

// (m*v, m) of node (gx,gy,gz) = what slow-path particles added to gin + the tiles of the work items that cover the node.
// A node with g = 4m + r along an axis lies in the tiles of blocks {m-1, m} (r < 3) or {m, m+1} (r = 3) on that axis:
// 8 candidate blocks per node, all among the 27 neighbours of the node's own block.  The wave first fetches the 27
// (first item, count) pairs with one load (lane i < 27), then every lane walks its 8 candidates in rounds so that the
// 8 tile loads of a round are in flight together.  The order of the sum is fixed; every staged value is read once.
// lane i < 27 fetches (first item, count) of neighbour block i of block (Bx,By,Bz); other lanes get (0,0)
__device__ __forceinline__ int2 neighbour_items(const MpmPtrs& S, int Bx, int By, int Bz) {
    const int lane = threadIdx.x & 63;
    int2 mine = make_int2(0, 0);
    if (lane < 27) {
        const int bx = Bx + lane / 9 - 1, by = By + (lane / 3) % 3 - 1, bz = Bz + lane % 3 - 1;
        if ((unsigned)bx < (unsigned)S.nbk && (unsigned)by < (unsigned)S.nbk && (unsigned)bz < (unsigned)S.nbk)
            mine = S.blk_items[(bx * S.nbk + by) * S.nbk + bz];
    }
    return mine;
}
// One axis of staged_index: tile coordinate t -> (first node of its sub-box, nodes in the sub-box, t - first)
__device__ __forceinline__ void staged_axis(int t, int& o, int& n, int& r) {
    o = (t == 0) ? 0 : (t <= 4 ? 1 : 5);
    n = (t == 0) ? 1 : (t <= 4 ? 4 : 3);
    r = t - o;
}
// RB = items per candidate block fetched in one go (8 x RB tile loads in flight).
//
// Round 6: this gather was written as if the grid kernel were latency-bound, and its counters say otherwise -- 816 VALU instructions per
// wave for ~10 float4 additions per lane: 3.7 waves per SIMD x 1.5 us of VALU issue at 1 M, FIFTEEN waves per SIMD on the reference's sand
// configuration (15 700 active blocks: 21 of the launch's 21 us).  What it spent them on: staged_index per candidate (~30 selects x 8), a
// branch + four zeroing moves around every predicated load, 64-bit address arithmetic, a 64-bit `live` word assembled bit by bit.  Now:
// staged_index taken apart by axis (six small selects per axis and side, ~6 multiply-adds per candidate); 32-bit element offsets from
// uniform bases; and NO predication -- a load that has nothing to fetch reads the all-zero tile at S.zero_off (or mask word 0, whose
// value is then ignored), so every lane issues the same 8 x RB loads and adds what comes back.  Adding +0 changes nothing and the order of
// the sum is still (round, candidate) whatever RB: every instantiation returns the bits it returned before.
// (Round 4 tried issuing the first round's tile loads TOGETHER with the mask loads and dropping unstored nodes afterwards --
// one dependent round trip fewer: 12.7 -> 15.5 us per launch at 1 M, the extra requests cost more than the trip saves;
// profiles/r4f_mpm_grid_speculative_tile_loads_rejected.txt.  The loads added here all hit ONE line.)
template <int RB>
__device__ __forceinline__ float4 gather_node(const MpmPtrs& S, int2 mine, int lx, int ly, int lz, float4 acc) {
    const int ax = (lx == 3) ? 0 : -1, ay = (ly == 3) ? 0 : -1, az = (lz == 3) ? 0 : -1;  // first candidate offset per axis
    // this node inside the tiles of the two candidate blocks per axis: coordinates t0 and t0 - 4
    const int t0x = lx - 4 * ax + 1, t0y = ly - 4 * ay + 1, t0z = lz - 4 * az + 1;
    int ox[2], nx[2], rx[2], oy[2], ny[2], ry[2], oz[2], nz[2], rz[2];
#pragma unroll
    for (int b = 0; b < 2; ++b) {
        staged_axis(t0x - 4 * b, ox[b], nx[b], rx[b]);
        staged_axis(t0y - 4 * b, oy[b], ny[b], ry[b]);
        staged_axis(t0z - 4 * b, oz[b], nz[b], rz[b]);
    }
    const int src0 = (ax + 1) * 9 + (ay + 1) * 3 + (az + 1);
    unsigned toff[8];  // in float4 units from S.part: first item * kTN + staged position of this node in that block's tiles
    unsigned moff[8];  // in 32-bit words from S.tile_mask: first item * 16 + the word that holds this node's bit
    int sh[8];         // ... and the bit inside it
    int nit[8];        // items of the candidate block
    int maxc = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        const int bx = c >> 2, by = (c >> 1) & 1, bz = c & 1;
        const int src = src0 + bx * 9 + by * 3 + bz;
        const int first = __shfl(mine.x, src), n = __shfl(mine.y, src);
        const int bit = ((t0x - 4 * bx) * kTS + (t0y - 4 * by)) * kTS + (t0z - 4 * bz);
        const int si = ox[bx] * 64 + nx[bx] * (oy[by] * 8 + ny[by] * oz[bz]) + (rx[bx] * ny[by] + ry[by]) * nz[bz] + rz[bz];   // = staged_index(tx, ty, tz)
        toff[c] = (unsigned)first * kTN + (unsigned)si;
        moff[c] = (unsigned)first * 16u + (unsigned)(bit >> 5);
        sh[c] = bit & 31;
        nit[c] = n;
        maxc = max(maxc, n);
    }
    const unsigned* __restrict__ mask32 = reinterpret_cast<const unsigned*>(S.tile_mask);   // (little-endian halves of the 64-bit words)
    const float4* __restrict__ part = S.part;
    const unsigned zero = S.zero_off;
    for (int r0 = 0; r0 < maxc; r0 += RB) {
        unsigned idx[RB][8];
        if (S.sparse_tiles) {                // (uniform)
            unsigned w[RB][8];
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) w[r][c] = mask32[(r0 + r < nit[c]) ? moff[c] + (unsigned)(r0 + r) * 16u : 0u];
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    const bool on = (r0 + r < nit[c]) && ((w[r][c] >> sh[c]) & 1u);
                    idx[r][c] = on ? toff[c] + (unsigned)(r0 + r) * kTN : zero;
                }
        } else {
#pragma unroll
            for (int r = 0; r < RB; ++r)
#pragma unroll
                for (int c = 0; c < 8; ++c) idx[r][c] = (r0 + r < nit[c]) ? toff[c] + (unsigned)(r0 + r) * kTN : zero;
        }
        float4 q[RB][8];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) q[r][c] = part[idx[r][c]];
#pragma unroll
        for (int r = 0; r < RB; ++r)
#pragma unroll
            for (int c = 0; c < 8; ++c) { acc.x += q[r][c].x; acc.y += q[r][c].y; acc.z += q[r][c].z; acc.w += q[r][c].w; }
    }
    return acc;
}

// grid_normalization_and_gravity (mpm_utils.py:398-409), add_damping_via_grid (:583-588) and every BC for ONE node of block
// (Bx,By,Bz), from its accumulated (m*v, m); returns grid_v_out
__device__ __forceinline__ float4 finish_node(const MpmPtrs& S, const StepParams& sp, const BCSet& bcs, float4 g, int ix, int iy, int iz) {
#pragma clang fp contract(off)
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (g.w > 1e-15f) {
        const float inv = 1.0f / g.w;
        v[0] = g.x * inv + sp.dt * sp.g[0];
        v[1] = g.y * inv + sp.dt * sp.g[1];
        v[2] = g.z * inv + sp.dt * sp.g[2];
    }
    if (sp.do_damping) { v[0] *= sp.damping; v[1] *= sp.damping; v[2] *= sp.damping; }
    for (int k = 0; k < bcs.n; ++k) apply_bc(bcs.bc[k], ix, iy, iz, S.ng, S.dx, sp.time, sp.dt, v);
    return make_float4(v[0], v[1], v[2], 0.0f);
}

// One WAVE updates the 4x4x4 nodes of active block `slot`: gather the staged tiles (+ what slow-path particles added to gin),
// normalise, gravity, damping, BCs -> dst.
template <int RB>
__device__ __forceinline__ void grid_block_update(const MpmPtrs& S, const StepParams& sp, const BCSet& bcs, int slot, float4* dst) {
    const int lane = threadIdx.x & 63;
#ifdef PIXIE_DIAG   // set_scalar "trace" 4: per active block four 100 MHz stamps -- start, neighbour row arrived, tiles summed, stored
#define PX_GRID_STAMP(i) do { if ((sp.trace & 4) && lane == 0 && slot < kMpmTraceItems) { asm volatile("s_waitcnt vmcnt(0)"); g_mpm_trace[slot * 8 + (i)] = wall_clock64(); } } while (0)
#else
#define PX_GRID_STAMP(i) do { } while (0)
#endif
    PX_GRID_STAMP(0);
    // one coalesced row: block id + the work items of the 27 neighbours (lane q holds neighbour q)
    const int2 row = (lane < 28) ? S.nbr_table[(size_t)slot * 28 + lane] : make_int2(0, 0);
    const int blk = __shfl(row.x, 0);
    PX_GRID_STAMP(1);
    int2 mine;
    mine.x = __shfl(row.x, (lane + 1) & 63); mine.y = __shfl(row.y, (lane + 1) & 63);
    const int Bz = blk % S.nbk, By = (blk / S.nbk) % S.nbk, Bx = blk / (S.nbk * S.nbk);
    // bit 0: active (set at re-binning); bit 1: slow-path particles added fp32 atomics into gin here
    const int flag = S.blk_flags[blk];
    const int lx = lane >> 4, ly = (lane >> 2) & 3, lz = lane & 3;
    const int ix = Bx * kBS + lx, iy = By * kBS + ly, iz = Bz * kBS + lz;
    const bool inside = ix < S.ng && iy < S.ng && iz < S.ng;
    const size_t idx = ((size_t)ix * S.ng + iy) * S.ng + iz;
    float4 g = gather_node<RB>(S, mine, lx, ly, lz, make_float4(0.f, 0.f, 0.f, 0.f));   // does not wait for the flag
    PX_GRID_STAMP(2);
    if (flag & 2) {
        if (inside) {
            const float4 q = S.gin[idx];
            g.x += q.x; g.y += q.y; g.z += q.z; g.w += q.w;
            S.gin[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
        if (lane == 0) S.blk_flags[blk] = flag & 1;
    }
    if (inside) dst[idx] = finish_node(S, sp, bcs, g, ix, iy, iz);
    PX_GRID_STAMP(3);
#ifdef PIXIE_DIAG
    if ((sp.trace & 4) && lane == 0 && slot < kMpmTraceItems)
        g_mpm_trace[slot * 8 + 6] = (unsigned long long)__builtin_amdgcn_s_getreg((31 << 11) | 4) | ((unsigned long long)__builtin_amdgcn_s_getreg((3 << 11) | 20) << 32);
#endif
}

// One wave per 4x4x4 block of nodes.  A block is ACTIVE when one of its 27 neighbours (itself included) holds particles.
// Only active blocks are read by the next G2P (a tile reaches one block beyond its own), so inactive blocks are skipped
// entirely (mode 0); their grid_v_out is brought up to date on demand (mode 1, used by the grid_v_out export) with the
// parameters of the last update, which for a massless node is just the BCs on v = 0.
// RB (tile loads in flight per candidate block) against occupancy.  The kernel is latency-bound -- a wave is three or four
// dependent memory round trips -- so what counts is how many waves are resident: a scene with several work items per block
// that fits in one round of waves (100 k particles in 50^3: 2200 active blocks) wants RB = 4 (189 VGPRs, 2 waves per SIMD); a
// scene with ~1.2 items per block and 9000 active blocks (1 M in 120^3) wants the registers back: RB = 1 = 101 VGPRs = 4 waves
// per SIMD, 14.9 -> 12.5 us per launch together with the sparse tiles.  (Holding the allocation to 80 / 64 VGPRs for 6 / 8 waves
// spills 22 / 39 dwords: 20.4 / 25.5 us.  profiles/r3s_mpm_grid_kernel_occupancy.txt)
// (Four active blocks per 256-thread workgroup instead of one wave per workgroup: measured equal at 3 700 active blocks in round 3 and again
// at the 15 700 of the reference's sand configuration in round 6 -- 21.99 vs 21.0 us, 102.0 vs 101.8 us per substep; the launch is not
// dispatch-bound.  profiles/r6c_sand_timing.txt)
template <int RB>
__global__ __launch_bounds__(64) void mpm_grid_block_kernel(MpmPtrs S, StepParams sp, BCSet bcs, int mode) {
    if (mode == 0) {
        grid_block_update<RB>(S, sp, bcs, (int)blockIdx.x, S.gout);
        return;
    }
    const int blk = (int)blockIdx.x;
    if (S.blk_flags[blk] & 1) return;
    const int Bz = blk % S.nbk, By = (blk / S.nbk) % S.nbk, Bx = blk / (S.nbk * S.nbk);
    const int lx = threadIdx.x >> 4, ly = (threadIdx.x >> 2) & 3, lz = threadIdx.x & 3;
    const int ix = Bx * kBS + lx, iy = By * kBS + ly, iz = Bz * kBS + lz;
    if (!(ix < S.ng && iy < S.ng && iz < S.ng)) return;
    S.gout[((size_t)ix * S.ng + iy) * S.ng + iz] = finish_node(S, sp, bcs, make_float4(0.f, 0.f, 0.f, 0.f), ix, iy, iz);
}

}  // namespace pixie
