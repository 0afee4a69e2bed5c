// pixie_amd/csrc/mpm_rebin_kernels.h -- MPM device code: re-binning of the particles by grid block (counting sort).
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// ------------------------------------------------------------------ re-binning (counting sort by block)
__device__ __forceinline__ int block_of(const MpmPtrs& S, int p) {
    int b[3];
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        int base = (int)(S.x[d * S.n + p] * S.inv_dx - 0.5f);
        base = max(0, min(base, S.ng - 3));
        b[d] = base / kBS;
    }
    return (b[0] * S.nbk + b[1]) * S.nbk + b[2];
}

// key[p] = block of particle p; rank[p] = its arrival number inside the block.  Lanes of a wave that share a key
// (the common case once the particles are binned) issue one atomic for the whole group.
__global__ __launch_bounds__(256) void bin_count_kernel(MpmPtrs S, int* __restrict__ keys, int* __restrict__ rank,
                                                        int* __restrict__ counts, unsigned* __restrict__ drift2_bits) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    const bool valid = p < S.n;
    const int key = valid ? block_of(S, p) : -1;
    {   // largest squared displacement since the last re-binning (drives the cadence, see rebin())
        float d2 = 0.0f;
        if (valid) {
            for (int d = 0; d < 3; ++d) { const float e = S.x[d * S.n + p] - S.xref[d * S.n + p]; d2 += e * e; }
            if (!(d2 < 3.0e38f)) d2 = 3.0e38f;
        }
        for (int off = 32; off > 0; off >>= 1) d2 = fmaxf(d2, __shfl_xor(d2, off, 64));
        if ((threadIdx.x & 63) == 0 && d2 > __uint_as_float(*drift2_bits)) atomicMax(drift2_bits, __float_as_uint(d2));
    }
    // Two groups of a wave share one atomic each -- the key of its first lane and the key of the first lane outside that group (binned
    // particles arrive block by block: a wave rarely spans more) -- and whoever is left takes its own.  All of a wave's atomics are
    // then in flight within three round trips; until round 6 every distinct key of the wave cost a dependent one (a scene in motion:
    // 4-6 per wave, 99 us for 1 M particles).  The arrival number is arbitrary either way; bin_local_order_kernel makes the order a
    // function of the particle data.
    const int lane = threadIdx.x & 63;
    int my_rank = 0;
    unsigned long long todo = __ballot(valid);
#pragma unroll
    for (int round = 0; round < 2; ++round) {
        if (!todo) break;
        const int leader = __ffsll((long long)todo) - 1;
        const int k = __shfl(key, leader);
        const unsigned long long grp = __ballot(valid && key == k) & todo;
        int base = 0;
        if (lane == leader) base = atomicAdd(&counts[k], __popcll(grp));
        base = __shfl(base, leader);
        if ((grp >> lane) & 1ull) my_rank = base + __popcll(grp & ((1ull << lane) - 1ull));
        todo &= ~grp;
    }
    if ((todo >> lane) & 1ull) my_rank = atomicAdd(&counts[key], 1);
    if (valid) { keys[p] = key; rank[p] = my_rank; }
}

// Exclusive scan of the block counts + the work list (<= cap particles per item), in three launches over chunks of 1024 blocks:
// chunk totals -> scan of the chunk totals (one workgroup) -> scan inside each chunk + the writes.  (Until round 5 ONE 1024-thread
// workgroup walked all blocks: 58 us for the 27 000 blocks of a 120^3 grid, 280 us for the 125 000 of the reference's sand configuration
// at n_grid 200 -- 7 % of that scene's run at a re-binning every ~33 substeps; profiles/r5last_stats_sand.csv.)
constexpr int kScanChunk = 1024;
__device__ __forceinline__ int wave_incl_scan(int v) {
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int off = 1; off < 64; off <<= 1) {
        const int o = __shfl_up(v, off, 64);
        if (lane >= off) v += o;
    }
    return v;
}
// exclusive prefix of v over the 1024-thread workgroup; *total = the workgroup's sum
__device__ __forceinline__ int wg_excl_scan_1024(int v, int* s_wave /* [16] */, int* total) {
    const int incl = wave_incl_scan(v);
    const int w = threadIdx.x >> 6;
    __syncthreads();
    if ((threadIdx.x & 63) == 63) s_wave[w] = incl;
    __syncthreads();
    int base = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < 16; ++k) { const int t = s_wave[k]; if (k < w) base += t; tot += t; }
    *total = tot;
    return base + incl - v;
}
__device__ __forceinline__ ScanTriple scan_triple_of(int c, int cap) {
    const int other = (cap == kWG) ? kWG / 2 : kWG;
    return ScanTriple{c, (c + cap - 1) / cap, (c + other - 1) / other};
}
__global__ __launch_bounds__(kScanChunk) void bin_scan_partial_kernel(const int* __restrict__ counts, ScanTriple* __restrict__ chunk, int nblocks, int cap) {
    __shared__ int s_w[3][16];
    const int b = blockIdx.x * kScanChunk + threadIdx.x;
    const ScanTriple t = scan_triple_of(b < nblocks ? counts[b] : 0, cap);
    int v[3] = {t.cnt, t.itm, t.other};
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        for (int off = 32; off > 0; off >>= 1) v[k] += __shfl_xor(v[k], off, 64);
        if ((threadIdx.x & 63) == 0) s_w[k][threadIdx.x >> 6] = v[k];
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        ScanTriple r{0, 0, 0};
        for (int w = 0; w < 16; ++w) { r.cnt += s_w[0][w]; r.itm += s_w[1][w]; r.other += s_w[2][w]; }
        chunk[blockIdx.x] = r;
    }
}
// chunk totals -> exclusive prefixes (in place); n_items[0] = work items, n_items[3] = what the other capacity would make.  One workgroup.
__global__ __launch_bounds__(1024) void bin_scan_chunks_kernel(ScanTriple* __restrict__ chunk, int nchunks, int* __restrict__ n_items) {
    __shared__ int s_w[16];
    const int per = (nchunks + 1023) / 1024;
    const int c0 = min((int)threadIdx.x * per, nchunks), c1 = min(c0 + per, nchunks);
    ScanTriple mine{0, 0, 0};
    for (int c = c0; c < c1; ++c) { mine.cnt += chunk[c].cnt; mine.itm += chunk[c].itm; mine.other += chunk[c].other; }
    int tc, ti, to;
    int pc = wg_excl_scan_1024(mine.cnt, s_w, &tc);
    int pi = wg_excl_scan_1024(mine.itm, s_w, &ti);
    int po = wg_excl_scan_1024(mine.other, s_w, &to);
    for (int c = c0; c < c1; ++c) {
        const ScanTriple t = chunk[c];
        chunk[c] = ScanTriple{pc, pi, po};
        pc += t.cnt; pi += t.itm; po += t.other;
    }
    if (threadIdx.x == 0) { n_items[0] = ti; n_items[3] = to; }
}
__global__ __launch_bounds__(kScanChunk) void bin_scan_write_kernel(const int* __restrict__ counts, const ScanTriple* __restrict__ chunk,
                                                                    int* __restrict__ offsets, int4* __restrict__ items,
                                                                    int2* __restrict__ blk_items, int nblocks, int cap) {
    __shared__ int s_w[16];
    const int b = blockIdx.x * kScanChunk + threadIdx.x;
    const int cnt = b < nblocks ? counts[b] : 0;
    const int nit = (cnt + cap - 1) / cap;
    const ScanTriple base = chunk[blockIdx.x];
    int dummy;
    const int c = base.cnt + wg_excl_scan_1024(cnt, s_w, &dummy);
    int i = base.itm + wg_excl_scan_1024(nit, s_w, &dummy);
    if (b >= nblocks) return;
    offsets[b] = c;
    blk_items[b] = make_int2(i, nit);
    for (int j = 0; j < cnt; j += cap) items[i++] = make_int4(b, c + j, min(cap, cnt - j), 0);
}

__global__ __launch_bounds__(256) void bin_order_kernel(const int* __restrict__ keys, const int* __restrict__ rank,
                                                        const int* __restrict__ offsets, int* __restrict__ order, int n) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p < n) order[offsets[keys[p]] + rank[p]] = p;
}

// Order inside a block: round-robin over its 64 cells -- position = (rank within the cell, cell).  Consecutive lanes of
// the block kernel then sit in consecutive cells, so the 27 same-offset LDS accesses of a wave (G2P reads and P2G
// ds_add_u64) hit distinct nodes in distinct banks instead of colliding 3-4 ways as they do in arrival order.
// One workgroup per block; `order` holds the block-contiguous listing, `order2` receives the final one.
//
// The rank within the cell is the particle's rank by its CURRENT SLOT among the block's particles of that cell -- not
// its arrival number (`order` is filled through atomics, so arrival differs from run to run).  That makes the listing,
// and with it the split of a crowded block into 256-particle work items and their fixed-point scales, a pure function
// of the particle data: together with the integer tile sums and the fixed summation order of the grid kernel, a rollout
// is bit-reproducible from run to run (as long as no particle takes the slow path's fp32 atomics).  Counting
// "same cell, lower slot" is quadratic in the block's population -- cnt^2 / 256 compares per thread through LDS tiles,
// ~20 us for the 800-particle blocks of the 100 k scene, once per re-binning.
__device__ __forceinline__ int cell_in_block(const MpmPtrs& S, int p) {
    int c = 0;
#pragma unroll
    for (int d = 0; d < 3; ++d) {
        int base = (int)(S.x[d * S.n + p] * S.inv_dx - 0.5f);
        base = max(0, min(base, S.ng - 3));
        c = c * kBS + (base & (kBS - 1));
    }
    return c;
}
// Material class of a particle for the ordering inside a block: the constitutive branches of return_map_and_stress.  A block
// that mixes materials (material_mode=neural uploads an id per particle, PG/material_field.py:343-363) is laid out class by
// class, round-robin by cell inside a class, so that a wave runs ONE branch instead of all of them (mixed 1 M scene: 1955 -> 1600
// VALU instructions per wave, 82.9 -> 78.5 us per substep = the single-material plastic scenes' 78.2; profiles/r5d_*); a
// single-material block -- every block of a single-material scene -- keeps the order it always had.
constexpr int kMatClasses = 7;
__device__ __forceinline__ int material_class(int material) {
    return material == 0 ? 0 : material == 1 ? 1 : material == 2 ? 2 : material == 3 ? 3 : material == 5 ? 4 : material == 6 ? 5 : 6;
}
__global__ __launch_bounds__(256) void bin_local_order_kernel(MpmPtrs S, const int* __restrict__ counts, const int* __restrict__ offsets,
                                                              const int* __restrict__ order, int* __restrict__ cellk,
                                                              int* __restrict__ rank, int* __restrict__ order2) {
    constexpr int kCells = kBS * kBS * kBS;
    __shared__ int cc[kMatClasses * kCells];     // particles per (class, cell)
    __shared__ int s_class_base[kMatClasses];
    __shared__ int2 s_tile[256];
    const int b = blockIdx.x;
    const int cnt = counts[b];
    if (cnt == 0) return;
    const int off = offsets[b];
    for (int t = threadIdx.x; t < kMatClasses * kCells; t += 256) cc[t] = 0;
    __syncthreads();
    for (int t = threadIdx.x; t < cnt; t += 256) {
        const int p = order[off + t];
        const int c = material_class(S.material[p]) * kCells + cell_in_block(S, p);   // key: (class, cell)
        cellk[off + t] = c;
        atomicAdd(&cc[c], 1);
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        int acc = 0;
        for (int m = 0; m < kMatClasses; ++m) {
            s_class_base[m] = acc;
            for (int k = 0; k < kCells; ++k) acc += cc[m * kCells + k];
        }
    }
    __syncthreads();
    for (int t0 = 0; t0 < cnt; t0 += 256) {
        const int t = t0 + threadIdx.x;
        const bool mine = t < cnt;
        const int c = mine ? cellk[off + t] : -1, p = mine ? order[off + t] : 0;
        int r = 0;
        for (int u0 = 0; u0 < cnt; u0 += 256) {
            __syncthreads();
            const int u = u0 + threadIdx.x;
            s_tile[threadIdx.x] = (u < cnt) ? make_int2(cellk[off + u], order[off + u]) : make_int2(-2, 0);
            __syncthreads();
            const int m = min(256, cnt - u0);
            for (int k = 0; k < m; ++k) {
                const int2 e = s_tile[k];
                r += (e.x == c && e.y < p) ? 1 : 0;
            }
        }
        if (mine) {      // slot = particles of earlier classes + (round r, cell) position inside the class
            const int m = c / kCells, cl = c - m * kCells;
            int pos = s_class_base[m];
            for (int k = 0; k < kCells; ++k) {
                const int n = cc[m * kCells + k];
                pos += min(n, r) + ((k < cl && n > r) ? 1 : 0);
            }
            order2[off + pos] = p;
        }
    }
}

// blk_flags bit 0 <- "one of my 27 neighbours holds particles", and the compact list of those ACTIVE blocks: the only
// ones the grid kernel is launched for (workgroup dispatch alone costs ~10 us for the 27000 blocks of a 120^3 grid).
__global__ __launch_bounds__(256) void bin_mark_active_kernel(const int* __restrict__ counts, int* __restrict__ blk_flags,
                                                              int* __restrict__ active_list, int* __restrict__ n_active, int nbk,
                                                              const int2* __restrict__ blk_items, int2* __restrict__ nbr_table) {
    const int b = blockIdx.x * 256 + threadIdx.x;
    if (b >= nbk * nbk * nbk) return;
    const int bz = b % nbk, by = (b / nbk) % nbk, bx = b / (nbk * nbk);
    bool active = false;
    for (int dx = -1; dx <= 1; ++dx)
        for (int dy = -1; dy <= 1; ++dy)
            for (int dz = -1; dz <= 1; ++dz) {
                const int x = bx + dx, y = by + dy, z = bz + dz;
                if ((unsigned)x < (unsigned)nbk && (unsigned)y < (unsigned)nbk && (unsigned)z < (unsigned)nbk)
                    active = active || counts[(x * nbk + y) * nbk + z] > 0;
            }
    blk_flags[b] = active ? 1 : 0;
    if (!active) return;
    const int slot = atomicAdd(n_active, 1);
    active_list[slot] = b;
    // everything the grid kernel needs to find this block's tiles, in one 224-byte row: one memory round trip there
    // instead of active_list -> blk_items -> tiles
    int2* row = nbr_table + (size_t)slot * 28;
    row[0] = make_int2(b, 0);
    for (int q = 0; q < 27; ++q) {
        const int x = bx + q / 9 - 1, y = by + (q / 3) % 3 - 1, z = bz + q % 3 - 1;
        const bool in = (unsigned)x < (unsigned)nbk && (unsigned)y < (unsigned)nbk && (unsigned)z < (unsigned)nbk;
        row[1 + q] = in ? blk_items[(x * nbk + y) * nbk + z] : make_int2(0, 0);
    }
}

// dst[r][q] = src[r][order[q]] for every row of the particle word array
// `skip_vcft`: the launch this re-binning precedes starts with a G2P, which overwrites v, C and F_trial of every particle that takes
// part (in the fused kernel they are not even stored between the gather and the scatter) -- 21 of the 51 rows are dead for those
// particles and only travel for the ones that sit out (selection != 0: deselected by the caller or frozen outside the grid), whose
// last stored values a caller may still read.
__global__ __launch_bounds__(256) void bin_permute_kernel(const unsigned* __restrict__ src, unsigned* __restrict__ dst,
                                                          const int* __restrict__ order, int n, int rows_per_y, int skip_vcft) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= n) return;
    const int p = order[q];
    const int r0 = blockIdx.y * rows_per_y, r1 = min(r0 + rows_per_y, (int)R_COUNT);
    const bool sits_out = skip_vcft && src[(size_t)R_SELECTION * n + p] != 0u;
    for (int r = r0; r < r1; ++r) {
        const bool dead = skip_vcft && ((r >= R_V && r < R_V + 3) || (r >= R_FT && r < R_FT + 9) || (r >= R_C && r < R_C + 9));
        if (dead && !sits_out) continue;
        const int rs = (r >= R_XREF) ? (R_X + r - R_XREF) : r;   // xref <- x: positions at this re-binning
        dst[(size_t)r * n + q] = src[(size_t)rs * n + p];
    }
}

__global__ void iota_kernel(int* dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = i;
}

}  // namespace pixie
