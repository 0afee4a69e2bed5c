// pixie_amd/csrc/mpm_types.h -- MPM solver: the types shared by the kernels, the host code and mpm_plan.h.
// The plain structs compile without HIP (g++ builds mpm_plan.h on them for tests/test_mpm_plan.py); MpmPtrs and staged_index need hipcc.
#pragma once

#include "mpm_math.h"

namespace pixie {

constexpr int kBS = 4;                    // cells per block edge (particles are binned by the block of their stencil base)
constexpr int kTS = 8;                    // tile nodes per edge: kBS + 2 (stencil reach) + 2 (one-cell drift margin each side)
constexpr int kTN = kTS * kTS * kTS;      // 512 nodes
static_assert(kTN == 512 && kTS == 8, "gather_node recovers the work item from a tile offset with >> 9 and packs tile coordinates in 3 bits");
constexpr int kWG = 256;                  // particles per work item / threads per workgroup (upper value)

// rows of the particle word array
enum Row {
    R_X = 0, R_V = 3, R_F = 6, R_FT = 15, R_C = 24, R_VOL = 33, R_MASS, R_DENSITY, R_E, R_NU, R_MU, R_LAM, R_BULK, R_YS,
    R_MATERIAL, R_SELECTION, R_PERM, R_XLO, R_XREF = R_XLO + 3, R_COUNT = R_XREF + 3
    // R_XLO: the low-order part of the position (set_scalar "compensated_x": x_true = x + xlo, |xlo| <= ulp(x)/2; zero otherwise);
    // R_XREF: position at the last re-binning (must stay the last rows: bin_permute_kernel fills them from x)
};
static_assert(R_COUNT == 51, "row table");

#if defined(__HIPCC__)
struct MpmPtrs {
    int n, ng, nbk;   // particles, grid nodes per axis, blocks per axis
    float dx, inv_dx;
    float *x, *v, *F, *Ft, *C;  // SoA: [3][n], [3][n], [9][n], [9][n], [9][n]
    float *vol, *mass, *density, *E, *nu, *mu, *lam, *bulk, *ys;
    int *material, *selection, *perm;
    float* xref;                 // [3][n] positions at the last re-binning (drift measurement)
    float* xlo;                  // [3][n] what the float32 position leaves behind (compensated_x), see particle_phase1
    float4 *gin, *gout;
    const int4* items;           // work list: (block id, first slot, count, 0)
    float4* part;                // [n_items][kTN]: (m*v.xyz, m) of each work item's tile, written by its P2G
    unsigned long long* tile_mask;  // [n_items][8]: bit t of a tile = "node t (tile coordinates, z fastest) is not all zero"
    unsigned zero_off;           // index (float4 units) of an all-zero tile behind the work items' tiles: what a gather reads where there is nothing to read
    int sparse_tiles;            // 1: P2G stores only the non-zero nodes of a tile and the grid kernel reads only those (masks);
                                 // 0: whole tiles both ways (scenes too small to be bandwidth-bound: one dependent load fewer)
    const int2* blk_items;       // per block: (first work item, number of work items)
    int* blk_flags;              // per block: bit 0 = active (particles nearby), bit 1 = slow-path particles wrote into gin here
    const int* active_list;      // the active blocks
    const int2* nbr_table;       // per active block (same order): [0] = (block id, 0), [1..27] = blk_items of its 27 neighbours
    const unsigned* staged_lut;  // [256]: staged_index of tile nodes t (low half) and t + 256 (high half)
    unsigned long long* oob;     // [0] particles skipped because their stencil left the grid, [1] slow-path particles,
                                 // [2] slow-path particles dropped because they had left every active block
};
#endif

struct StepParams {
    float dt, time;
    float g[3];
    float damping;
    int do_damping;
    float rpic;
    int xcd_order;  // set_scalar "xcd_order": work items dealt to the XCDs in contiguous runs (see mpm_block_kernel)
    int comp_x;     // set_scalar "compensated_x": carry the rounding error of x += dt v in xlo (see particle_phase1)
    int trace;      // timing studies: bit 0 = workgroups stamp s_memrealtime around their phases into g_mpm_trace;
                    // bits 8.. = ablations for bottleneck hunting (RESULTS ARE WRONG with any of them set):
                    // 0x100 skip the LDS scatter atomics, 0x200 skip the workgroup scale reduction (fixed scale),
                    // 0x400 skip the tile staging loads, 0x800 skip the tile publish stores
    MaterialScalars ms;
};

struct BCDev {
    int type, surface_type, reset, pad;
    float point[3], size[3], velocity[3], normal[3];
    float start, end, friction;
};
constexpr int kMaxBCPerLaunch = 16;
struct BCSet {
    int n;
    BCDev bc[kMaxBCPerLaunch];
};

struct PModDev {
    int type;
    float point[3], force[3], velocity[3], normal[3], h1[3], h2[3];
    float rot_scale, trans_scale, start, end;
    const int* mask;   // [n] in the CALLER's particle order (index through perm)
};
constexpr int kMaxPModFused = 8;
struct PModSet {
    int n;
    PModDev pm[kMaxPModFused];
};

struct ScanTriple { int cnt, itm, other; };   // particles, work items at `cap`, work items at the other capacity (auto item_cap, see rebin())
struct FrameXform { float shift[3]; float inv_scale; float mean[3]; float inv_scale2; float M[9]; };   // the export transform (make_frame_xform)
constexpr int kMaxBatch = 32;   // scenes per batched launch (mpm_batch_kernels.h)

#if defined(__HIPCC__)
// Position of tile node (lx,ly,lz) inside a STAGED tile (part[item][512]).  A tile starts one node before its block, so
// along each axis its 8 nodes fall into three grid blocks: {0}, {1..4}, {5..7}.  The staged tile is stored sub-box by
// sub-box (27 boxes of 1|4|3 nodes per axis, each contiguous) so that the grid kernel, whose wave owns one 4x4x4 grid
// block, reads ONE contiguous run per covering tile instead of 16 64-byte rows scattered over 128-byte lines
// (measured: 3x over-fetch with the plain row-major tile).
__host__ __device__ __forceinline__ int staged_index(int lx, int ly, int lz) {
    const int sx = (lx == 0) ? 0 : (lx <= 4 ? 1 : 2), sy = (ly == 0) ? 0 : (ly <= 4 ? 1 : 2), sz = (lz == 0) ? 0 : (lz <= 4 ? 1 : 2);
    const int ox = (sx == 0) ? 0 : (sx == 1 ? 1 : 5), oy = (sy == 0) ? 0 : (sy == 1 ? 1 : 5), oz = (sz == 0) ? 0 : (sz == 1 ? 1 : 5);
    const int ny = (sy == 0) ? 1 : (sy == 1 ? 4 : 3), nz = (sz == 0) ? 1 : (sz == 1 ? 4 : 3);
    // nodes in the sub-boxes that precede (sx,sy,sz): full x-slabs, then full y-rows of this slab, then z-boxes of this row
    const int nx = (sx == 0) ? 1 : (sx == 1 ? 4 : 3);
    const int before = ox * 64 + nx * (oy * 8 + ny * oz);
    return before + ((lx - ox) * ny + (ly - oy)) * nz + (lz - oz);
}
#endif

}  // namespace pixie
