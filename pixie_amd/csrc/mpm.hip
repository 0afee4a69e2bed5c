// pixie_amd/csrc/mpm.hip -- MLS-MPM substep for MI355X (gfx950) behind the pixie_mpm_* C ABI.
//
// Replaces the reference's Warp launch sequence MPM_Simulator_WARP.p2g2p
// (third_party/PhysGaussian/mpm_solver_warp/mpm_solver_warp.py:514-637):
//   zero_grid -> pre-P2G modifiers -> compute_stress_from_F_trial -> p2g_apic_with_stress ->
//   grid_normalization_and_gravity -> add_damping_via_grid -> BC collide x k -> g2p
// (6-10 launches + 5 forced device syncs per substep) by TWO launches per substep and no syncs:
//
//   block kernel <G2P,P2G>:  G2P of substep t  ->  modifiers, return map + stress, P2G of
//                            substep t+1.  F_trial, stress, C' and the new v never leave registers
//                            between the gather and the scatter (in the fused form v and C are not
//                            even stored: nothing reads them before the next G2P overwrites them).
//   grid kernel:             normalise + gravity + damping + every BC in one sweep, and
//                            clears (m, m*v) behind itself so no separate zero_grid runs.
//
// Particles are kept binned by 4x4x4-cell grid block (counting sort every `resort_interval`
// substeps, all on the device).  One workgroup serves <= 256 particles of one block: it stages the
// block's 8x8x8 node neighbourhood of grid velocities in LDS (one coalesced pass), every particle
// gathers its 27 nodes from LDS, scatters its 27 x (m*v, m) contributions with LDS float atomics
// (ds_add_f32) into a second LDS tile, and the workgroup flushes the tile's non-zero nodes to HBM with
// one global fp32 atomic per word: ~2k global atomics per workgroup instead of 27.6k.  A particle whose
// stencil has drifted out of its workgroup's tile (stale binning) takes a slow path straight to
// global memory, so correctness never depends on the binning being fresh.
//
// Layout in HBM: particle state is SoA fp32/int32 rows of one [45][n] word array (each row a fully
// coalesced 256 B/wave stream; two copies, ping-ponged by the re-binning permutation); the grid is two
// float4 arrays: gin = (m*v.xyz, m) that P2G accumulates, gout = (v.xyz, 0) that G2P gathers.  `perm`
// maps internal slots to the caller's particle order; every import/export goes through it.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "mpm_math.h"
#include "splat_math.h"

// One translation unit (the kernels are compiled where they are launched, and this file's name carries its compile flag in build.py),
// in files by concern.  This one: the solo handle, its launch sequencing and the C API.
#include "mpm_types.h"               // shared types
#include "mpm_plan.h"                // the host's decisions as pure functions (tests/test_mpm_plan.py)
// device code, in the definition order of the code object
#include "mpm_particle_kernels.h"
#include "mpm_rebin_kernels.h"
#include "mpm_grid_kernels.h"
#include "mpm_batch_kernels.h"
#include "mpm_dense_grid_kernels.h"
#include "mpm_setup_kernels.h"
#include "mpm_export_kernels.h"

namespace pixie {
#ifdef PIXIE_DIAG
int mpm_trace_read(unsigned long long* host, int n_words) {
    return (int)hipMemcpyFromSymbol(host, HIP_SYMBOL(g_mpm_trace), (size_t)n_words * sizeof(unsigned long long));
}
#endif
}  // namespace pixie

// ====================================================================== host side
using namespace pixie;

// What a re-binning reads back (pinned; the copies of rebin() fill one group of fields each from its device-side producer)
struct RebinReadback {
    struct Counts {                      // d_n_items[0..3], as bin_scan_chunks_kernel / bin_mark_active_kernel / bin_count_kernel leave them
        int n_items, n_active;
        float drift2;                    // largest squared particle drift since the last re-binning
        int n_items_other;               // work items at the other capacity (128 <-> 256)
    } counts;
    unsigned long long slow_total;       // oob[1]
    struct { float lo, hi; } mass;       // d_mass_range[0..1]
    unsigned long long left_grid;        // oob[0]
    unsigned long long left_blocks;      // oob[2]
};
static_assert(sizeof(RebinReadback::Counts) == 4 * sizeof(int), "d_n_items is four 32-bit words");

struct pixie_mpm {
    MpmPtrs S{};
    double grid_lim = 1.0;
    double time = 0.0;
    // host mirror of MPMModelStruct scalars (mpm_solver_warp.py:74-92)
    float g[3] = {0, 0, 0};
    float rpic = 0.0f, damping = 1.1f;
    MaterialScalars ms{};
    std::vector<pixie_bc_desc> bcs;          // host copies; cuboid points advance like `modify` (:899-905)
    std::vector<BCDev> bcs_dev;              // float versions (what the kernels see)
    std::vector<PModDev> pmods;
    std::vector<int*> masks;
    float* init_cov = nullptr;               // [n][6], caller order
    // particle word array [R_COUNT][n], two copies ping-ponged by the re-binning permutation
    unsigned* words[2] = {nullptr, nullptr};
    int cur = 0;
    // re-binning scratch
    int nblocks = 0;
    int *keys = nullptr, *rank = nullptr, *counts = nullptr, *offsets = nullptr, *order = nullptr, *order2 = nullptr, *d_n_items = nullptr;
    int4* items = nullptr;
    RebinReadback* readback = nullptr;       // pinned
    int n_items = 0;
    bool needs_sort = true;                  // positions changed behind the binning's back (or never binned)
    int resort_interval = 4, steps_since_sort = 0;  // starts cautious, doubles while the measured drift allows
    bool xref_valid = false;
    int trace = 0;
    bool resort_auto = true;                 // adapt resort_interval to the observed drift (off once the caller sets it)
    unsigned long long slow_at_rebin = 0;
    unsigned long long lost_seen = 0;        // oob[0] + oob[2] as read back at the last re-binning
    int2* blk_items = nullptr;               // per block: (first work item, item count)
    int occupancy = 5;                       // register-allocation target of the fused kernel (waves per SIMD): 5 or 6
    int item_cap = kWG;                      // particles per work item of the current binning: 128 or 256
    int item_cap_user = 0;                   // set_scalar "item_cap": 0 = automatic
    bool auto_half_items = false;            // item_cap "auto": 128-thread work items from the next re-binning on (see rebin())
    int comp_x = 0;                          // set_scalar "compensated_x"
    int xcd_order = 1;                       // set_scalar "xcd_order" (on: 63.5 -> 61.9 us per substep at 1 M, 18.0 -> 17.5 at 100 k, same bits; profiles/r5g_xcd_order.txt)
    bool pmods_were_active = false;
    float4* part = nullptr;                  // staged tiles of the last P2G, [max_items][kTN]
    unsigned long long* tile_mask = nullptr; // [max_items][8] occupancy bits of the staged tiles
    int grid_rb = 0;                         // grid kernel: tile loads in flight per candidate block (0 = by scene size; 1, 2, 4)
    ScanTriple* scan_chunks = nullptr;       // [ceil(nblocks / 1024)] re-binning scan scratch
    int sparse = -1;                         // sparse tile publishing: -1 auto (on when the work list exceeds two items per CU), 0, 1
    bool pending_p2g = false;                // staged tiles not yet consumed by the grid kernel
    int* blk_flags = nullptr;
    int* active_list = nullptr;              // blocks with particles in their 27-neighbourhood (built at re-binning)
    int2* nbr_table = nullptr;               // 28 int2 per active block (see MpmPtrs)
    int scatter_bits = 32;                   // mode in force: 32 = packed pairs of 32-bit sums, 2 LDS atomics per node; 64 = exact 64-bit fixed point, 4 per node
    int scatter_bits_user = 0;               // 0 (default): chosen by the particle-mass contrast at every re-binning (below); 32 / 64: forced
    bool mass_range_dirty = true;            // masses changed since the contrast was last measured
    unsigned* d_mass_range = nullptr;        // [0] min, [1] max of the positive particle masses, as float bits
    float mass_contrast = 1.0f;              // max / min as of the last measurement
    int wide = -1;                           // -1 auto: the latency-optimised variant when the scene cannot fill the chip; 0/1 forced
    int n_cus = 256;
    int n_active = 0;
    bool gout_sparse = false;                // inactive blocks of gout are stale (refreshed on export)
    StepParams last_grid_sp{};
    std::vector<BCDev> last_grid_bcs;
    long n_sorts = 0;
    std::vector<void*> allocs;
    std::vector<void*> grid_allocs;          // everything sized by n_grid (re-made by pixie_mpm_regrid)
    bool dirty_grid = false;                 // gin holds an un-consumed P2G (phase API)
    // profiling
    bool profile = false;
    std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_particle, ev_grid;
};

namespace {

template <typename T>
int dev_alloc(pixie_mpm* h, T** ptr, size_t count, bool grid_sized = false) {
    void* p = nullptr;
    PX_CHECK_HIP(hipMalloc(&p, count * sizeof(T)));
    (grid_sized ? h->grid_allocs : h->allocs).push_back(p);
    PX_CHECK_HIP(hipMemset(p, 0, count * sizeof(T)));
    *ptr = static_cast<T*>(p);
    return 0;
}

// point the row pointers of h->S at the current copy of the word array
void bind_rows(pixie_mpm* h) {
    MpmPtrs& S = h->S;
    const size_t n = (size_t)S.n;
    float* f = reinterpret_cast<float*>(h->words[h->cur]);
    int* i = reinterpret_cast<int*>(h->words[h->cur]);
    S.x = f + R_X * n; S.v = f + R_V * n; S.F = f + R_F * n; S.Ft = f + R_FT * n; S.C = f + R_C * n;
    S.vol = f + R_VOL * n; S.mass = f + R_MASS * n; S.density = f + R_DENSITY * n; S.E = f + R_E * n; S.nu = f + R_NU * n;
    S.mu = f + R_MU * n; S.lam = f + R_LAM * n; S.bulk = f + R_BULK * n; S.ys = f + R_YS * n;
    S.material = i + R_MATERIAL * n; S.selection = i + R_SELECTION * n; S.perm = i + R_PERM * n; S.xref = f + R_XREF * n; S.xlo = f + R_XLO * n;
    S.items = h->items; S.part = h->part; S.tile_mask = h->tile_mask; S.blk_items = h->blk_items; S.blk_flags = h->blk_flags; S.active_list = h->active_list; S.nbr_table = h->nbr_table;
}

// counts -> offsets, work list, per-block item ranges (three scan launches), active blocks + their neighbour rows
void build_work_list(pixie_mpm* h, hipStream_t st) {
    const int nchunks = cdiv(h->nblocks, kScanChunk);
    hipLaunchKernelGGL(bin_scan_partial_kernel, dim3(nchunks), dim3(kScanChunk), 0, st, h->counts, h->scan_chunks, h->nblocks, h->item_cap);
    hipLaunchKernelGGL(bin_scan_chunks_kernel, dim3(1), dim3(1024), 0, st, h->scan_chunks, nchunks, h->d_n_items);
    hipLaunchKernelGGL(bin_scan_write_kernel, dim3(nchunks), dim3(kScanChunk), 0, st, h->counts, h->scan_chunks, h->offsets, h->items, h->blk_items,
                       h->nblocks, h->item_cap);
    (void)hipMemsetAsync(h->d_n_items + 1, 0, sizeof(int), st);
    hipLaunchKernelGGL(bin_mark_active_kernel, dim3(cdiv(h->nblocks, 256)), dim3(256), 0, st, h->counts, h->blk_flags, h->active_list,
                       h->d_n_items + 1, h->S.nbk, h->blk_items, h->nbr_table);  // (rewrites every flag: no slow-path writes are pending here)
}

// Re-bin the particles by grid block (counting sort) and rebuild the work list.  Everything runs on the device;
// the host only waits for the 4-byte item count so that the block kernel gets an exact grid.
int rebin(pixie_mpm* h, hipStream_t st, bool g2p_follows = false) {
    MpmPtrs& S = h->S;
    const int n = S.n;
    // Work-item capacity: 256 particles (one per thread).  128-thread items were measured too (set_scalar "item_cap"):
    // 100 k particles 21.0 -> 23.8 us per launch (916 items instead of 526: the per-item tile staging / barriers /
    // publish dominate), 1 M particles 100 -> 95 us but the grid kernel pays for twice the tiles (14.8 -> 20.7 us).
    // Automatic: 128-thread items in scenes so sparse that few blocks hold more than 128 particles -- there a 256-thread
    // workgroup runs two waves without a particle (the reference's sand configuration at 1 M: 120 -> 108 us per substep) -- and
    // 256 everywhere else (1 M in 120^3: 62.5 vs 70.9 us; 100 k in 50^3: 17.5 vs 21.8; profiles/r5e_item_cap_sparse_scenes.txt).
    // Decided from the block histogram of THIS re-binning (both item counts come back with it; if the choice flips, only the work
    // list is built again -- three small launches): see below.
    h->item_cap = h->item_cap_user > 0 ? h->item_cap_user : (h->auto_half_items ? kWG / 2 : kWG);
    RebinReadback* rb = h->readback;
    PX_CHECK_HIP(hipMemsetAsync(h->counts, 0, (size_t)h->nblocks * sizeof(int), st));
    PX_CHECK_HIP(hipMemsetAsync(h->d_n_items + 2, 0, sizeof(int), st));
    hipLaunchKernelGGL(bin_count_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, S, h->keys, h->rank, h->counts,
                       reinterpret_cast<unsigned*>(h->d_n_items + 2));
    build_work_list(h, st);
    hipLaunchKernelGGL(bin_order_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, h->keys, h->rank, h->offsets, h->order, n);
    // keys/rank are free again: reuse them as the local kernel's scratch
    hipLaunchKernelGGL(bin_local_order_kernel, dim3((unsigned)h->nblocks), dim3(256), 0, st, S, h->counts, h->offsets, h->order, h->keys,
                       h->rank, h->order2);
    const int rows_per_y = 9;
    hipLaunchKernelGGL(bin_permute_kernel, dim3(cdiv(n, 256), cdiv(R_COUNT, rows_per_y)), dim3(256), 0, st,
                       h->words[h->cur], h->words[h->cur ^ 1], h->order2, n, rows_per_y, g2p_follows ? 1 : 0);
    PX_CHECK_HIP(hipGetLastError());
    const bool measure_mass = h->mass_range_dirty;
    if (measure_mass) {
        PX_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)h->d_mass_range, (int)0xffffffffu, 1, st));
        PX_CHECK_HIP(hipMemsetD32Async((hipDeviceptr_t)(h->d_mass_range + 1), 0, 1, st));
        hipLaunchKernelGGL(mass_range_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, S, h->d_mass_range);
        PX_CHECK_HIP(hipMemcpyAsync(&rb->mass, h->d_mass_range, sizeof rb->mass, hipMemcpyDeviceToHost, st));
    }
    PX_CHECK_HIP(hipMemcpyAsync(&rb->counts, h->d_n_items, sizeof rb->counts, hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipMemcpyAsync(&rb->slow_total, h->S.oob + 1, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipMemcpyAsync(&rb->left_grid, h->S.oob, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipMemcpyAsync(&rb->left_blocks, h->S.oob + 2, sizeof(unsigned long long), hipMemcpyDeviceToHost, st));
    PX_CHECK_HIP(hipStreamSynchronize(st));
    // particles lost so far (left the grid / left every active block), as of this re-binning: free to read, no extra sync
    h->lost_seen = rb->left_grid + rb->left_blocks;
    h->n_items = rb->counts.n_items;
    h->n_active = rb->counts.n_active;
    if (h->item_cap == kWG || h->item_cap == kWG / 2) {
        const long other = rb->counts.n_items_other;
        const long n256 = (h->item_cap == kWG) ? h->n_items : other, n128 = (h->item_cap == kWG) ? other : h->n_items;
        h->auto_half_items = half_items_wanted(h->auto_half_items, n128, n256);
        const int want = h->auto_half_items ? kWG / 2 : kWG;
        if (h->item_cap_user == 0 && want != h->item_cap) {   // in force from THIS binning: rebuild the work list for the other capacity
            h->item_cap = want;
            build_work_list(h, st);
            PX_CHECK_HIP(hipMemcpyAsync(&rb->counts, h->d_n_items, 2 * sizeof(int), hipMemcpyDeviceToHost, st));   // (n_items, n_active)
            PX_CHECK_HIP(hipStreamSynchronize(st));
            h->n_items = rb->counts.n_items;
            h->n_active = rb->counts.n_active;
        }
    }
    if (measure_mass) {
        h->mass_contrast = mass_contrast_of(rb->mass.lo, rb->mass.hi);
        h->mass_range_dirty = false;
    }
    // (like sparse_tiles: decided at a re-binning only -- the mode changes how a tile is summed in LDS, not what is published)
    h->scatter_bits = scatter_bits_for(h->scatter_bits_user, h->mass_contrast);
    // (decided here and only here: never between a P2G and the grid kernel that consumes its tiles)
    S.sparse_tiles = h->sparse >= 0 ? h->sparse : (grid_crowded(h->n_active, h->n_cus) ? 1 : 0);
    // Cadence from the measured drift and slow-path share of the interval just finished (next_resort_interval)
    if (h->resort_auto) {
        const unsigned long long since = rb->slow_total - h->slow_at_rebin;
        h->slow_at_rebin = rb->slow_total;
        const double drift_cells = sqrt((double)rb->counts.drift2) * (double)S.inv_dx;
        if (h->n_sorts > 0 && h->xref_valid) h->resort_interval = next_resort_interval(h->resort_interval, drift_cells, since, n);
        h->xref_valid = true;
    }
    h->cur ^= 1;
    bind_rows(h);
    h->needs_sort = false;
    h->steps_since_sort = 0;
    ++h->n_sorts;
    return 0;
}

StepParams make_params(const pixie_mpm* h, double dt, double time) {
    StepParams sp{};
    sp.dt = (float)dt;
    sp.time = (float)time;
    for (int d = 0; d < 3; ++d) sp.g[d] = h->g[d];
    sp.damping = h->damping;
    sp.do_damping = (h->damping < 1.0f) ? 1 : 0;  // gate mpm_solver_warp.py:595
    sp.rpic = h->rpic;
    sp.trace = h->trace;
    sp.comp_x = h->comp_x;
    sp.xcd_order = h->xcd_order;
    sp.ms = h->ms;
    return sp;
}

struct FieldInfo { void* ptr; int k; bool is_int; bool soa; };

bool find_field(pixie_mpm* h, const std::string& name, FieldInfo* fi) {
    MpmPtrs& S = h->S;
    struct Row { const char* nm; void* p; int k; bool is_int; };
    const Row rows[] = {
        {"x", S.x, 3, false}, {"v", S.v, 3, false}, {"F", S.F, 9, false}, {"F_trial", S.Ft, 9, false},
        {"C", S.C, 9, false}, {"vol", S.vol, 1, false}, {"mass", S.mass, 1, false}, {"density", S.density, 1, false},
        {"E", S.E, 1, false}, {"nu", S.nu, 1, false}, {"mu", S.mu, 1, false}, {"lam", S.lam, 1, false},
        {"bulk", S.bulk, 1, false}, {"yield_stress", S.ys, 1, false},
        {"material", S.material, 1, true}, {"selection", S.selection, 1, true},
    };
    for (const Row& r : rows)
        if (name == r.nm) { *fi = FieldInfo{r.p, r.k, r.is_int, true}; return true; }
    return false;
}

BCSet make_bcset(const pixie_mpm* h, size_t first) { return pixie::make_bcset(h->bcs_dev, first); }
void advance_bcs(pixie_mpm* h, double dt) { advance_bcs_state(h->time, h->bcs, h->bcs_dev, dt); }
FusedVariant fused_variant(const pixie_mpm* h) { return pixie::fused_variant(h->wide, h->n_items, h->n_cus, h->occupancy, h->scatter_bits); }

// The one table of block-kernel variants: (g2p, p2g, fused variant, packed scatter, trace) -> the template arguments <G, P, OCC, FL>,
// handed to launch.run<G, P, OCC, FL>().  The solo launch (mpm_block_kernel, below) and the batched one (mpm_block_batch_kernel,
// mpm_batch_host.h) both read it: the variants round differently (test_latency_optimised_variant_matches), so a scene must get the
// same one either way.  The F_TRACE pair (timing studies) exists for a Launch with kHasTrace in the PIXIE_DIAG build only.
template <class Launch>
void dispatch_block_variant(bool g2p, bool p2g, FusedVariant fv, bool pack, bool trace, const Launch& launch) {
    if (g2p && p2g) {
#ifdef PIXIE_DIAG
        if constexpr (Launch::kHasTrace) {
            if (trace && pack) return launch.template run<true, true, 5, F_TRACE | F_PACK32>();
            if (trace) return launch.template run<true, true, 5, F_TRACE>();
        }
#endif
        if (fv == FV_WIDE && pack) launch.template run<true, true, 2, F_WIDE | F_PACK32>();
        else if (fv == FV_WIDE) launch.template run<true, true, 2, F_WIDE>();
        else if (fv == FV_SIX_WAVES) launch.template run<true, true, 6, 0>();
        else if (pack) launch.template run<true, true, 5, F_PACK32>();
        else launch.template run<true, true, 5, 0>();
    } else if (g2p) {
        launch.template run<true, false, 5, 0>();
    } else if (pack) {
        launch.template run<false, true, 5, F_PACK32>();
    } else {
        launch.template run<false, true, 5, 0>();
    }
}

struct SoloBlockLaunch {
    static constexpr bool kHasTrace = true;
    const pixie_mpm* h;
    hipStream_t st;
    const StepParams& sp;
    const PModSet& pms;
    template <bool G, bool P, int OCC, int FL>
    void run() const {
        hipLaunchKernelGGL((mpm_block_kernel<G, P, OCC, FL>), dim3((unsigned)std::max(h->n_items, 1)), dim3(h->item_cap), 0, st, h->S, sp, pms);
    }
};

// A substep's launches are split in two: the PLAN part (every decision and every change of host state: re-binning, cadence, modifier
// selection, parameters, BC motion, time) and the ISSUE part (the launches).  pixie_mpm_step runs both per handle; pixie_mpm_batch_step
// runs the plan of every scene and issues one launch for all of them.
struct ParticlePlan {
    bool g2p = false, p2g = false;
    bool run = false;          // something to launch (no work items: nothing binned)
    bool fused_mods = true;    // <= kMaxPModFused active modifiers: applied inside the block kernel
    StepParams sp{};
    PModSet pms{};
    std::vector<PModDev> ordered;
};

int plan_particle(pixie_mpm* h, bool g2p, bool p2g, const StepParams& sp, hipStream_t st, ParticlePlan& pl) {
    // (never while staged tiles are waiting for the grid kernel: the work list they are indexed by must not change)
    if (!h->pending_p2g && (h->needs_sort || (h->resort_interval > 0 && h->steps_since_sort >= h->resort_interval)))
        if (rebin(h, st, g2p)) return 1;
    if (g2p) ++h->steps_since_sort;
    pl.g2p = g2p; pl.p2g = p2g; pl.sp = sp; pl.pms = PModSet{};
    // modifiers whose time window cannot contain this substep are dropped on the host
    pl.ordered = active_pmods(h->pmods, sp.time);
    if (h->resort_auto && !pl.ordered.empty() && !h->pmods_were_active)   // a modifier switches on: velocities may jump
        h->resort_interval = std::min(h->resort_interval, 4);
    h->pmods_were_active = !pl.ordered.empty();
    pl.fused_mods = pl.ordered.size() <= (size_t)kMaxPModFused;
    if (pl.fused_mods) {
        pl.pms.n = (int)pl.ordered.size();
        for (int k = 0; k < pl.pms.n; ++k) pl.pms.pm[k] = pl.ordered[k];
    }
    pl.run = h->n_items != 0;  // no particles binned (n_particles > 0 always gives >= 1 item)
    if (pl.run && p2g) h->pending_p2g = true;
    return 0;
}

int issue_particle(pixie_mpm* h, const ParticlePlan& pl, hipStream_t st) {
    if (!pl.run) return 0;
    const bool g2p = pl.g2p, p2g = pl.p2g;
    const StepParams& sp = pl.sp;
    const int blocks = cdiv(h->S.n, 256);
    const bool pack = h->scatter_bits == 32, trace = (h->trace & ~4) != 0;
    const FusedVariant fv = fused_variant(h);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->profile && p2g && g2p) {
        PX_CHECK_HIP(hipEventCreate(&e0)); PX_CHECK_HIP(hipEventCreate(&e1));
        PX_CHECK_HIP(hipEventRecord(e0, st));
    }
    if (g2p && p2g && pl.fused_mods) {
        dispatch_block_variant(true, true, fv, pack, trace, SoloBlockLaunch{h, st, sp, pl.pms});
    } else {
        if (g2p) {
            PModSet none{};
            dispatch_block_variant(true, false, fv, pack, trace, SoloBlockLaunch{h, st, sp, none});
        }
        if (p2g) {
            if (!pl.fused_mods) {
                for (const PModDev& m : pl.ordered)
                    hipLaunchKernelGGL(pmod_kernel, dim3(blocks), dim3(256), 0, st, h->S, sp, m);
            }
            dispatch_block_variant(false, true, fv, pack, trace, SoloBlockLaunch{h, st, sp, pl.pms});
        }
    }
    if (e0) {
        PX_CHECK_HIP(hipEventRecord(e1, st));
        h->ev_particle.emplace_back(e0, e1);
    }
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_particle(pixie_mpm* h, bool g2p, bool p2g, const StepParams& sp, hipStream_t st) {
    static thread_local ParticlePlan pl;   // (re-used: no allocation per launch on the solo path)
    if (plan_particle(h, g2p, p2g, sp, st, pl)) return 1;
    return issue_particle(h, pl, st);
}

void launch_grid_blocks(const pixie_mpm* h, hipStream_t st, const StepParams& sp, const BCSet& set, int mode, int n_wg) {
    const int rb = h->grid_rb > 0 ? h->grid_rb : (grid_crowded(h->n_active, h->n_cus) ? 1 : 4);
    const dim3 g((unsigned)n_wg), b(64);
    if (rb == 1) hipLaunchKernelGGL(mpm_grid_block_kernel<1>, g, b, 0, st, h->S, sp, set, mode);
    else if (rb == 2) hipLaunchKernelGGL(mpm_grid_block_kernel<2>, g, b, 0, st, h->S, sp, set, mode);
    else hipLaunchKernelGGL(mpm_grid_block_kernel<4>, g, b, 0, st, h->S, sp, set, mode);
}

// One launch of a grid update: the active-block kernel (mode 0 = update, 1 = refresh the inactive blocks) or the dense kernel
struct GridOp {
    bool blocks;
    int mode;        // blocks: mode; dense: normalise
    int n_wg;        // blocks: workgroups
    BCSet set;
};
struct GridPlan {
    StepParams sp{};
    std::vector<GridOp> ops;
    // the common case, and the only one pixie_mpm_batch_step issues batched: one active-block update with every BC
    bool single_block_update() const { return ops.size() == 1 && ops[0].blocks && ops[0].mode == 0; }
};

int plan_grid(pixie_mpm* h, const StepParams& sp, double dt, GridPlan& gp) {
    gp.sp = sp;
    gp.ops.clear();
    const size_t nbc = h->bcs_dev.size();
    size_t done = 0;
    int normalise = 1;
    do {
        const BCSet set = make_bcset(h, done);
        if (normalise && h->pending_p2g && nbc <= (size_t)kMaxBCPerLaunch) {
            // staged tiles of the last P2G + slow-path atomics in gin; blocks with nothing nearby are skipped
            gp.ops.push_back(GridOp{true, 0, std::max(h->n_active, 1), set});
            h->gout_sparse = true;
            h->last_grid_sp = sp;
            h->last_grid_bcs.assign(h->bcs_dev.begin(), h->bcs_dev.end());
        } else if (normalise && h->pending_p2g) {  // more BCs than one launch carries: dense follow-up passes need every block
            gp.ops.push_back(GridOp{true, 0, std::max(h->n_active, 1), set});
            gp.ops.push_back(GridOp{true, 1, h->nblocks, set});
            h->gout_sparse = false;
        } else {                          // nothing staged (or a further pass of BCs over gout)
            gp.ops.push_back(GridOp{false, normalise, 0, set});
            if (normalise) h->gout_sparse = false;
        }
        done += set.n;
        normalise = 0;
    } while (done < nbc);
    h->pending_p2g = false;
    advance_bcs(h, dt);
    return 0;
}

int issue_grid(pixie_mpm* h, const GridPlan& gp, hipStream_t st) {
    const long total = (long)h->S.ng * h->S.ng * h->S.ng;
    const int blocks = cdiv(total, 256);
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (h->profile) {
        PX_CHECK_HIP(hipEventCreate(&e0)); PX_CHECK_HIP(hipEventCreate(&e1));
        PX_CHECK_HIP(hipEventRecord(e0, st));
    }
    for (const GridOp& op : gp.ops) {
        if (op.blocks) launch_grid_blocks(h, st, gp.sp, op.set, op.mode, op.n_wg);
        else hipLaunchKernelGGL(mpm_grid_kernel, dim3(blocks), dim3(256), 0, st, h->S, gp.sp, op.set, op.mode);
    }
    if (e0) {
        PX_CHECK_HIP(hipEventRecord(e1, st));
        h->ev_grid.emplace_back(e0, e1);
    }
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int launch_grid(pixie_mpm* h, const StepParams& sp, double dt, hipStream_t st) {
    static thread_local GridPlan gp;       // (re-used: no allocation per launch on the solo path)
    if (plan_grid(h, sp, dt, gp)) return 1;
    return issue_grid(h, gp, st);
}

// Everything whose size depends on n_grid: the two grid arrays, the block tables and the work list / staged tiles.
// Used by pixie_mpm_create and by pixie_mpm_regrid (set_parameters_dict changing n_grid / grid_lim after the particles
// were loaded, mpm_solver_warp.py:315-342: the reference re-allocates the grids and recomputes dx, nothing else).
// The new buffers are allocated first; the old ones are released only when every allocation succeeded, so a failed
// regrid leaves the handle as it was.
int alloc_grid(pixie_mpm* h, int n_grid, double grid_lim) {
    MpmPtrs& S = h->S;
    const int nbk = (n_grid + kBS - 1) / kBS;
    const int nblocks = nbk * nbk * nbk;
    const size_t n = (size_t)S.n, G = (size_t)n_grid * n_grid * n_grid;
    const size_t max_items = (n + 63) / 64 + std::min<size_t>((size_t)nblocks, n);   // for the smallest capacity (64)
    // gather_node (grid kernel) forms tile offsets item * kTN in 32-bit arithmetic: 8.4 M work items, i.e. > 100 M particles
    // at the smallest capacity, would wrap silently -- refused here instead
    PX_REQUIRE(max_items * (size_t)kTN < ((size_t)1 << 32), "pixie_mpm: %zu work items exceed the 32-bit tile offsets of the grid kernel (2^23 items)", max_items);
    std::vector<void*> old;
    old.swap(h->grid_allocs);
    float4 *gin = nullptr, *gout = nullptr, *part = nullptr;
    unsigned long long* tile_mask = nullptr;
    int *counts = nullptr, *offsets = nullptr, *active_list = nullptr, *blk_flags = nullptr;
    int4* items = nullptr;
    int2 *nbr_table = nullptr, *blk_items = nullptr;
    int rc = 0;
    rc |= dev_alloc(h, &gin, G, true); rc |= dev_alloc(h, &gout, G, true);
    rc |= dev_alloc(h, &counts, (size_t)nblocks, true); rc |= dev_alloc(h, &offsets, (size_t)nblocks, true);
    rc |= dev_alloc(h, &items, max_items, true);
    rc |= dev_alloc(h, &active_list, (size_t)nblocks, true);
    rc |= dev_alloc(h, &nbr_table, (size_t)nblocks * 28, true);
    rc |= dev_alloc(h, &blk_items, (size_t)nblocks, true); rc |= dev_alloc(h, &blk_flags, (size_t)nblocks, true);
    ScanTriple* scan_chunks = nullptr;
    rc |= dev_alloc(h, &scan_chunks, (size_t)cdiv(nblocks, kScanChunk), true);
    rc |= dev_alloc(h, &part, (max_items + 1) * kTN, true);     // (+ the zero tile of gather_node; dev_alloc clears, nothing ever writes it)
    rc |= dev_alloc(h, &tile_mask, max_items * 8, true);
    if (rc) {   // keep the old grid
        for (void* p : h->grid_allocs) (void)hipFree(p);
        h->grid_allocs.swap(old);
        return 1;
    }
    for (void* p : old) (void)hipFree(p);
    S.ng = n_grid;
    h->grid_lim = grid_lim;
    S.dx = (float)(grid_lim / n_grid);              // mpm_solver_warp.py:62-66, :320-326
    S.inv_dx = (float)((double)n_grid / grid_lim);
    S.nbk = nbk;
    h->nblocks = nblocks;
    S.gin = gin; S.gout = gout;
    h->counts = counts; h->offsets = offsets; h->items = items; h->active_list = active_list; h->nbr_table = nbr_table;
    h->blk_items = blk_items; h->blk_flags = blk_flags; h->part = part; h->tile_mask = tile_mask;
    S.zero_off = (unsigned)(max_items * kTN);
    h->scan_chunks = scan_chunks;
    h->n_items = 0; h->n_active = 0;
    h->auto_half_items = false;
    h->needs_sort = true; h->xref_valid = false;
    h->pending_p2g = false; h->dirty_grid = false; h->gout_sparse = false;
    if (h->resort_auto) h->resort_interval = 4;
    return rc;
}

}  // namespace

#include "mpm_batch_host.h"

extern "C" {

// mpm_solver_warp.py:84-86, 391-393: the reference evaluates `wp.sin` / `wp.sqrt` from Python scope, i.e. Warp's float32
// built-ins (float32 argument and result); the products around them are Python doubles and the struct member is float32.
static float host_alpha(double friction_angle) {
    const double sin_phi = (double)sinf((float)(friction_angle / 180.0 * 3.14159265));
    return (float)((double)sqrtf((float)(2.0 / 3.0)) * 2.0 * sin_phi / (3.0 - sin_phi));
}

int pixie_mpm_create(pixie_mpm** out, int n_particles, int n_grid, double grid_lim) {
    PX_REQUIRE(out && n_particles > 0 && n_grid >= 4 && grid_lim > 0, "pixie_mpm_create: bad arguments");
    pixie_mpm* h = new pixie_mpm();
    MpmPtrs& S = h->S;
    S.n = n_particles;
    const size_t n = (size_t)n_particles;
    int rc = 0;
    rc |= dev_alloc(h, &h->words[0], (size_t)R_COUNT * n); rc |= dev_alloc(h, &h->words[1], (size_t)R_COUNT * n);
    rc |= dev_alloc(h, &S.oob, 3);
    {
        unsigned* lut = nullptr;
        rc |= dev_alloc(h, &lut, (size_t)kWG);
        if (!rc) {
            unsigned host[kWG];
            for (int t = 0; t < kWG; ++t) {
                const int a = t, b = t + kWG;
                host[t] = (unsigned)staged_index(a >> 6, (a >> 3) & 7, a & 7) | ((unsigned)staged_index(b >> 6, (b >> 3) & 7, b & 7) << 16);
            }
            if (hipMemcpy(lut, host, sizeof host, hipMemcpyHostToDevice) != hipSuccess) rc = 1;
        }
        S.staged_lut = lut;
    }
    rc |= dev_alloc(h, &h->keys, n); rc |= dev_alloc(h, &h->rank, n); rc |= dev_alloc(h, &h->order, n); rc |= dev_alloc(h, &h->order2, n);
    rc |= dev_alloc(h, &h->d_n_items, 4);
    rc |= dev_alloc(h, &h->d_mass_range, 2);
    rc |= alloc_grid(h, n_grid, grid_lim);
    rc |= dev_alloc(h, &h->init_cov, 6 * n);
    if (rc) { pixie_mpm_destroy(h); return 1; }
    if (hipHostMalloc((void**)&h->readback, sizeof(RebinReadback)) != hipSuccess) { pixie_mpm_destroy(h); return set_error("hipHostMalloc failed"); }
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0) h->n_cus = cus;
    }
    bind_rows(h);
    hipLaunchKernelGGL(iota_kernel, dim3(cdiv(n, 256)), dim3(256), 0, 0, S.perm, n_particles);
    hipLaunchKernelGGL(identity_F_kernel, dim3(cdiv(n, 256)), dim3(256), 0, 0, S.Ft, n_particles);  // :272-277
    PX_CHECK_HIP(hipDeviceSynchronize());
    // defaults of initialize(), mpm_solver_warp.py:74-92
    h->ms.plastic_viscosity = 0.0f; h->ms.softening = 0.1f; h->ms.hardening = 0.0f; h->ms.xi = 0.0f;
    h->ms.alpha = host_alpha(25.0);
    h->rpic = 0.0f; h->damping = 1.1f;
    *out = h;
    return 0;
}

int pixie_mpm_destroy(pixie_mpm* h) {
    if (!h) return 0;
    for (void* p : h->allocs) (void)hipFree(p);
    for (void* p : h->grid_allocs) (void)hipFree(p);
    for (int* m : h->masks) (void)hipFree(m);
    if (h->readback) (void)hipHostFree(h->readback);
    for (auto& e : h->ev_particle) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    for (auto& e : h->ev_grid) { (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second); }
    delete h;
    return 0;
}

int pixie_mpm_regrid(pixie_mpm* h, int n_grid, double grid_lim, void* stream) {
    PX_REQUIRE(h && n_grid >= 4 && grid_lim > 0, "pixie_mpm_regrid: bad arguments");
    PX_REQUIRE(!h->dirty_grid, "pixie_mpm_regrid: a phase-API P2G is pending");
    PX_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));   // nothing may still be reading the old grid
    if (alloc_grid(h, n_grid, grid_lim)) return 1;
    bind_rows(h);
    hipLaunchKernelGGL(unfreeze_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S.selection, h->S.n);
    h->mass_range_dirty = true;   // re-admitted particles count towards the mass contrast again
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_set_field(pixie_mpm* h, const char* name, const void* d_src, int64_t count, void* stream) {
    PX_REQUIRE(h && name && d_src, "pixie_mpm_set_field: null argument");
    hipStream_t st = as_stream(stream);
    const std::string nm(name);
    const int n = h->S.n;
    if (nm == "init_cov") {
        PX_REQUIRE(count == (int64_t)n * 6, "set_field(init_cov): expected %lld scalars, got %lld", (long long)n * 6, (long long)count);
        PX_CHECK_HIP(hipMemcpyAsync(h->init_cov, d_src, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    FieldInfo fi;
    PX_REQUIRE(find_field(h, nm, &fi), "set_field: unknown field '%s'", name);
    PX_REQUIRE(count == (int64_t)n * fi.k, "set_field(%s): expected %lld scalars, got %lld", name, (long long)n * fi.k, (long long)count);
    if (nm == "mass" || nm == "selection") { h->mass_range_dirty = true; h->needs_sort = true; }
    if (nm == "material") h->needs_sort = true;     // the order inside a block goes by material class
    if (nm == "x") {   // positions replaced: binning stale, frozen particles get another chance
        h->needs_sort = true; h->xref_valid = false; h->resort_interval = h->resort_auto ? 4 : h->resort_interval;
        h->auto_half_items = false;   // a new scene decides its work-item capacity afresh, like a new handle
        hipLaunchKernelGGL(unfreeze_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, h->S.selection, n);
        h->mass_range_dirty = true;   // re-admitted particles count towards the mass contrast again
        PX_CHECK_HIP(hipMemsetAsync(h->S.xlo, 0, (size_t)3 * n * sizeof(float), st));   // new positions carry no remainder
    }
    if (fi.is_int)
        hipLaunchKernelGGL(aos_to_soa_kernel<int>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const int*)d_src, (int*)fi.ptr, n, fi.k, h->S.perm);
    else
        hipLaunchKernelGGL(aos_to_soa_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)d_src, (float*)fi.ptr, n, fi.k, h->S.perm);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_get_field(pixie_mpm* h, const char* name, void* d_dst, int64_t count, void* stream) {
    PX_REQUIRE(h && name && d_dst, "pixie_mpm_get_field: null argument");
    hipStream_t st = as_stream(stream);
    const std::string nm(name);
    const int n = h->S.n;
    const long G = (long)h->S.ng * h->S.ng * h->S.ng;
    if (nm == "grid_m" || nm == "grid_v_in" || nm == "grid_v_out") {
        const int k = (nm == "grid_m") ? 1 : 3;
        PX_REQUIRE(count == (int64_t)G * k, "get_field(%s): expected %lld scalars, got %lld", name, (long long)G * k, (long long)count);
        const float4* src = (nm == "grid_v_out") ? h->S.gout : h->S.gin;
        if (nm == "grid_v_out" && h->gout_sparse) {  // bring the skipped (massless, far from any particle) blocks up to date
            BCSet set{};
            set.n = (int)h->last_grid_bcs.size();
            for (int k = 0; k < set.n; ++k) set.bc[k] = h->last_grid_bcs[k];
            launch_grid_blocks(h, st, h->last_grid_sp, set, 1, h->nblocks);
            h->gout_sparse = false;
        }
        if (nm != "grid_v_out" && h->pending_p2g)
            hipLaunchKernelGGL(grid_export_pending_kernel, dim3((unsigned)h->nblocks), dim3(64), 0, st, h->S, (float*)d_dst, nm == "grid_m" ? 0 : 1);
        else
            hipLaunchKernelGGL(grid_export_kernel, dim3(cdiv(G, 256)), dim3(256), 0, st, src, (float*)d_dst, G, nm == "grid_m" ? 0 : 1);
        PX_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (nm == "stress") {
        PX_REQUIRE(count == (int64_t)n * 9, "get_field(stress): expected %lld scalars", (long long)n * 9);
        hipLaunchKernelGGL(stress_export_kernel, dim3(cdiv(n, 256)), dim3(256), 0, st, h->S, (float*)d_dst, h->S.perm);
        PX_CHECK_HIP(hipGetLastError());
        return 0;
    }
    if (nm == "init_cov") {
        PX_REQUIRE(count == (int64_t)n * 6, "get_field(init_cov): expected %lld scalars", (long long)n * 6);
        PX_CHECK_HIP(hipMemcpyAsync(d_dst, h->init_cov, (size_t)n * 6 * sizeof(float), hipMemcpyDeviceToDevice, st));
        return 0;
    }
    if (nm == "cov") return pixie_mpm_export_cov(h, (float*)d_dst, stream);
    FieldInfo fi;
    PX_REQUIRE(find_field(h, nm, &fi), "get_field: unknown field '%s'", name);
    PX_REQUIRE(count == (int64_t)n * fi.k, "get_field(%s): expected %lld scalars, got %lld", name, (long long)n * fi.k, (long long)count);
    if (fi.is_int)
        hipLaunchKernelGGL(soa_to_aos_kernel<int>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const int*)fi.ptr, (int*)d_dst, n, fi.k, h->S.perm);
    else
        hipLaunchKernelGGL(soa_to_aos_kernel<float>, dim3(cdiv(n, 256)), dim3(256), 0, st, (const float*)fi.ptr, (float*)d_dst, n, fi.k, h->S.perm);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_fill_field(pixie_mpm* h, const char* name, double value, void* stream) {
    PX_REQUIRE(h && name, "pixie_mpm_fill_field: null argument");
    FieldInfo fi;
    PX_REQUIRE(find_field(h, name, &fi), "fill_field: unknown field '%s'", name);
    const long cnt = (long)h->S.n * fi.k;
    if (fi.is_int)
        hipLaunchKernelGGL(fill_kernel<int>, dim3(cdiv(cnt, 256)), dim3(256), 0, as_stream(stream), (int*)fi.ptr, cnt, (int)value);
    else
        hipLaunchKernelGGL(fill_kernel<float>, dim3(cdiv(cnt, 256)), dim3(256), 0, as_stream(stream), (float*)fi.ptr, cnt, (float)value);
    PX_CHECK_HIP(hipGetLastError());
    if (std::string(name) == "material") h->needs_sort = true;
    return 0;
}

int pixie_mpm_set_scalar(pixie_mpm* h, const char* key, double value) {
    PX_REQUIRE(h && key, "pixie_mpm_set_scalar: null argument");
    const std::string k(key);
    if (k == "rpic_damping") h->rpic = (float)value;
    else if (k == "grid_v_damping_scale") h->damping = (float)value;
    else if (k == "hardening") h->ms.hardening = (float)value;
    else if (k == "xi") h->ms.xi = (float)value;
    else if (k == "softening") h->ms.softening = (float)value;
    else if (k == "plastic_viscosity") h->ms.plastic_viscosity = (float)value;
    else if (k == "friction_angle") h->ms.alpha = host_alpha(value);  // mpm_solver_warp.py:390-393
    else if (k == "gx") h->g[0] = (float)value;
    else if (k == "gy") h->g[1] = (float)value;
    else if (k == "gz") h->g[2] = (float)value;
    else if (k == "time") h->time = value;
#ifdef PIXIE_DIAG
    else if (k == "profile") h->profile = value != 0.0;
#else
    else if (k == "profile" || k == "trace") {   // switching them OFF is a no-op everywhere (callers written against the round-4 library do that)
        if (value != 0.0) return set_error("pixie_mpm_set_scalar(%s): diagnostic switch, only in the PIXIE_DIAG build (libpixie_hip_diag.so)", key);
    }
#endif
    else if (k == "scatter_bits") {
        PX_REQUIRE(value == 64 || value == 32 || value == 0, "scatter_bits must be 0 (auto: by mass contrast), 64 (exact) or 32 (packed pairs)");
        h->scatter_bits_user = (int)value;
        if (value != 0) h->scatter_bits = (int)value; else { h->mass_range_dirty = true; h->needs_sort = true; }
    }
    else if (k == "grid_rb") { PX_REQUIRE(value == 0 || value == 1 || value == 2 || value == 4, "grid_rb must be 0, 1, 2 or 4"); h->grid_rb = (int)value; }
    else if (k == "sparse_tiles") { PX_REQUIRE(value == -1 || value == 0 || value == 1, "sparse_tiles must be -1 (auto), 0 or 1"); h->sparse = (int)value; h->needs_sort = true; }
    else if (k == "wide") { PX_REQUIRE(value == -1 || value == 0 || value == 1, "wide must be -1 (auto), 0 or 1"); h->wide = (int)value; }
#ifdef PIXIE_DIAG
    else if (k == "trace") h->trace = (int)value;
#endif
    else if (k == "compensated_x") h->comp_x = value != 0.0 ? 1 : 0;
    else if (k == "xcd_order") h->xcd_order = value != 0.0 ? 1 : 0;
    else if (k == "occupancy") { PX_REQUIRE(value == 5 || value == 6, "occupancy must be 5 or 6 waves per SIMD"); h->occupancy = (int)value; }
    else if (k == "item_cap") { PX_REQUIRE(value == 0 || value == 64 || value == 128 || value == 192 || value == 256, "item_cap must be 0 (auto), 64, 128, 192 or 256"); h->item_cap_user = (int)value; h->needs_sort = true; }
    else if (k == "resort_interval") { h->resort_interval = (int)value; h->resort_auto = false; }   // substeps between re-binnings (0 = only when positions are replaced)
    else return set_error("set_scalar: unknown key '%s'", key);
    return 0;
}

int pixie_mpm_get_scalar(pixie_mpm* h, const char* key, double* value) {
    PX_REQUIRE(h && key && value, "pixie_mpm_get_scalar: null argument");
    const std::string k(key);
    if (k == "time") *value = h->time;
    else if (k == "dx") *value = h->S.dx;
    else if (k == "inv_dx") *value = h->S.inv_dx;
    else if (k == "alpha") *value = h->ms.alpha;
    else if (k == "rpic_damping") *value = h->rpic;
    else if (k == "grid_v_damping_scale") *value = h->damping;
    else if (k == "resort_interval") *value = h->resort_interval;
    else if (k == "n_work_items") *value = h->n_items;
    else if (k == "item_cap") *value = h->item_cap;                    // the capacity in force (as of the last re-binning when auto)
    else if (k == "scatter_bits") *value = h->scatter_bits;            // the mode in force (as of the last re-binning when auto)
    else if (k == "scatter_bits_user") *value = h->scatter_bits_user;
    else if (k == "mass_contrast") *value = h->mass_contrast;
    else if (k == "n_active_blocks") *value = h->n_active;
    else if (k == "n_rebins") *value = (double)h->n_sorts;
    else if (k == "lost_particles_seen") *value = (double)h->lost_seen;   // as of the last re-binning; does not synchronise
    else if (k == "dropped_particles") {  // slow-path particles that had left every active block; synchronises the device
        unsigned long long v = 0;
        PX_CHECK_HIP(hipMemcpy(&v, h->S.oob + 2, sizeof v, hipMemcpyDeviceToHost));
        *value = (double)v;
    }
    else if (k == "slow_path_particles") {  // synchronises the device
        unsigned long long v = 0;
        PX_CHECK_HIP(hipMemcpy(&v, h->S.oob + 1, sizeof v, hipMemcpyDeviceToHost));
        *value = (double)v;
    }
    else return set_error("get_scalar: unknown key '%s'", key);
    return 0;
}

int pixie_mpm_update_mass(pixie_mpm* h, void* stream) {
    PX_REQUIRE(h, "null handle");
    h->mass_range_dirty = true; h->needs_sort = true;
    hipLaunchKernelGGL(mass_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_finalize_mu_lam(pixie_mpm* h, int with_bulk, void* stream) {
    PX_REQUIRE(h, "null handle");
    hipLaunchKernelGGL(mu_lam_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, with_bulk);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_apply_additional_params(pixie_mpm* h, const double point[3], const double size[3], double E, double nu,
                                      double density, int material, void* stream) {
    PX_REQUIRE(h && point && size, "null argument");
    const float3 pt = make_float3((float)point[0], (float)point[1], (float)point[2]);
    const float3 sz = make_float3((float)size[0], (float)size[1], (float)size[2]);
    hipLaunchKernelGGL(additional_params_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, pt, sz,
                       (float)E, (float)nu, (float)density, material);
    PX_CHECK_HIP(hipGetLastError());
    h->needs_sort = true;      // materials changed: the order inside a block goes by material class
    return 0;
}

int pixie_mpm_apply_additional_params_batch(pixie_mpm* h, int64_t n_boxes, const float* d_boxes, const float* d_params,
                                            const int32_t* d_material, void* stream) {
    PX_REQUIRE(h && n_boxes >= 0 && (n_boxes == 0 || (d_boxes && d_params && d_material)), "apply_additional_params_batch: bad arguments");
    if (n_boxes == 0) return 0;
    hipLaunchKernelGGL(additional_params_batch_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, (long)n_boxes, d_boxes,
                       d_params, reinterpret_cast<const int*>(d_material));
    PX_CHECK_HIP(hipGetLastError());
    h->needs_sort = true;      // materials changed: the order inside a block goes by material class
    return 0;
}

int pixie_mpm_add_bc(pixie_mpm* h, const pixie_bc_desc* bc) {
    PX_REQUIRE(h && bc, "null argument");
    PX_REQUIRE(bc->type >= 0 && bc->type <= 2, "add_bc: unknown type %d", bc->type);
    h->bcs.push_back(*bc);
    h->bcs_dev.push_back(to_dev(*bc));
    return 0;
}

int pixie_mpm_add_particle_modifier(pixie_mpm* h, const pixie_pmod_desc* pm, void* stream) {
    PX_REQUIRE(h && pm, "null argument");
    PX_REQUIRE(pm->type >= 0 && pm->type <= 2, "add_particle_modifier: unknown type %d", pm->type);
    PModDev m{};
    m.type = pm->type;
    for (int d = 0; d < 3; ++d) {
        m.point[d] = (float)pm->point[d]; m.force[d] = (float)pm->force[d]; m.velocity[d] = (float)pm->velocity[d];
        m.normal[d] = (float)pm->normal[d]; m.h1[d] = (float)pm->h1[d]; m.h2[d] = (float)pm->h2[d];
    }
    m.rot_scale = (float)pm->rotation_scale; m.trans_scale = (float)pm->translation_scale;
    m.start = (float)pm->start_time; m.end = (float)pm->end_time;
    int* mask = nullptr;
    PX_CHECK_HIP(hipMalloc(&mask, (size_t)h->S.n * sizeof(int)));
    h->masks.push_back(mask);
    m.mask = mask;
    const float3 size = make_float3((float)pm->size[0], (float)pm->size[1], (float)pm->size[2]);
    hipLaunchKernelGGL(select_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, m, size,
                       (float)pm->half_height, (float)pm->radius, mask);
    PX_CHECK_HIP(hipGetLastError());
    h->pmods.push_back(m);
    return 0;
}

// (Round 4 captured the steady part of this loop -- 32 substeps of grid kernel + fused block kernel -- as a HIP graph, replayed
// whenever nothing the kernels compute depended on the time inside the chunk.  Bit-identical, and no faster: 18.00 vs 18.10 us
// per substep at 100 k particles, 63.8 vs 63.2 at 1 M; with several scenes sharing the GPU it was slower (two 1 M scenes: 128.8
// vs 109.8 us per pair of substeps).  The host already runs far ahead of the device, so what a substep pays at its two kernel
// boundaries is the device's own 3.6 us, graph or not.  profiles/r4h_mpm_step_graph_rejected.txt)
int pixie_mpm_step(pixie_mpm* h, double dt, int n_substeps, void* stream) {
    PX_REQUIRE(h && n_substeps >= 0, "pixie_mpm_step: bad arguments");
    if (n_substeps == 0) return 0;
    PX_REQUIRE(!h->dirty_grid, "pixie_mpm_step: a phase-API P2G is pending; finish the substep with phases 1,2 first");
    hipStream_t st = as_stream(stream);
    // substep 0: modifiers + stress + P2G at time t0
    if (launch_particle(h, false, true, make_params(h, dt, h->time), st)) return 1;
    for (int i = 0; i < n_substeps; ++i) {
        if (launch_grid(h, make_params(h, dt, h->time), dt, st)) return 1;
        h->time = h->time + dt;  // mpm_solver_warp.py:637
        const bool last = (i == n_substeps - 1);
        // G2P of substep i fused with modifiers/stress/P2G of substep i+1 (evaluated at the new time)
        if (launch_particle(h, true, !last, make_params(h, dt, h->time), st)) return 1;
    }
    return 0;
}

int pixie_mpm_batch_create(pixie_mpm_batch** out, pixie_mpm* const* handles, int n_handles) {
    PX_REQUIRE(out, "pixie_mpm_batch_create: null output pointer");
    *out = nullptr;
    PX_REQUIRE(handles, "pixie_mpm_batch_create: null handle list");
    PX_REQUIRE(n_handles >= 1 && n_handles <= kMaxBatch, "pixie_mpm_batch_create: %d scenes; a batch holds 1 ... %d", n_handles, kMaxBatch);
    for (int i = 0; i < n_handles; ++i) {
        PX_REQUIRE(handles[i], "pixie_mpm_batch_create: scene %d is a null handle", i);
        for (int j = 0; j < i; ++j) PX_REQUIRE(handles[j] != handles[i], "pixie_mpm_batch_create: scenes %d and %d are the same handle", j, i);
    }
    for (int i = 0; i < n_handles; ++i)
        if (batch_check_handle(handles[i], i, "pixie_mpm_batch_create")) return 1;
    pixie_mpm_batch* b = new pixie_mpm_batch();
    b->h.assign(handles, handles + n_handles);
    b->n_cus = handles[0]->n_cus;
    if (hipGetDevice(&b->device) != hipSuccess ||
        hipEventCreateWithFlags(&b->ev_up[0], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b->ev_up[1], hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&b->finished, hipEventDisableTiming) != hipSuccess) {
        pixie_mpm_batch_destroy(b);
        return set_error("pixie_mpm_batch_create: hipEventCreate failed");
    }
    *out = b;
    return 0;
}

// Bit for bit what pixie_mpm_step(h, dt, n_substeps, stream) does to each scene alone: the same plan (plan_particle / plan_grid, in
// the same order per scene), the same kernel bodies, the same per-scene parameters; only the launches are shared.
int pixie_mpm_batch_step(pixie_mpm_batch* b, double dt, int n_substeps, void* stream) {
    PX_REQUIRE(b && n_substeps >= 0, "pixie_mpm_batch_step: bad arguments");
    if (n_substeps == 0) return 0;
    const int ns = (int)b->h.size();
    for (int s = 0; s < ns; ++s)
        if (batch_check_handle(b->h[s], s, "pixie_mpm_batch_step")) return 1;
    int dev = -1;
    PX_CHECK_HIP(hipGetDevice(&dev));
    PX_REQUIRE(dev == b->device, "pixie_mpm_batch_step: HIP device %d is current, the batch was created on device %d", dev, b->device);
    // one chunk of n_substeps for every scene: the launches of the scheduler's common case
    BatchSched q;
    q.dt = dt; q.chunk = n_substeps; q.n_chunks = 1; q.total = n_substeps;
    return batch_schedule(b, std::vector<BatchSched>(ns, q), std::vector<BatchExport>(), std::vector<BatchSplat>(), as_stream(stream));
}

// Per-scene dt, substep counts and frame exports: each scene s runs, bit for bit, its solo frame loop
//   for f < n_chunks: [pixie_mpm_export_frame(frame f) if n_out > 0]; pixie_mpm_step(dt, steps_per_chunk)
// with the launches shared across scenes (batch_schedule).
int pixie_mpm_batch_run(pixie_mpm_batch* b, const pixie_batch_sched* per_scene, int n_scenes, void* stream) {
    return pixie_mpm_batch_run_splats(b, per_scene, nullptr, n_scenes, stream);
}

// pixie_mpm_batch_run, with the scenes that have splats[s] set exporting (pos, cov, log-scales, quaternions) per frame, bit for
// bit as pixie_mpm_export_frame_splats in their solo loop.  splats == NULL, or no scene with splats: pixie_mpm_batch_run's launches.
int pixie_mpm_batch_run_splats(pixie_mpm_batch* b, const pixie_batch_sched* per_scene, const pixie_batch_splat_out* splats, int n_scenes,
                               void* stream) {
    PX_REQUIRE(b && per_scene, "pixie_mpm_batch_run: null argument");
    const int ns = (int)b->h.size();
    PX_REQUIRE(n_scenes == ns, "pixie_mpm_batch_run: %d schedules for a batch of %d scenes", n_scenes, ns);
    std::vector<BatchSched> sc(ns);
    std::vector<BatchExport> ex(ns);
    memset(ex.data(), 0, ex.size() * sizeof(BatchExport));
    std::vector<BatchSplat> spl(ns, BatchSplat{nullptr, nullptr});
    for (int s = 0; s < ns; ++s) {
        const pixie_batch_sched& q = per_scene[s];
        const pixie_mpm* h = b->h[s];
        PX_REQUIRE(std::isfinite(q.dt) && q.dt > 0.0, "pixie_mpm_batch_run: scene %d: dt %g (a positive finite time step is required)", s, q.dt);
        PX_REQUIRE(q.steps_per_chunk >= 0 && q.n_chunks >= 0, "pixie_mpm_batch_run: scene %d: negative counts (%d substeps per chunk, %d chunks)",
                   s, q.steps_per_chunk, q.n_chunks);
        PX_REQUIRE((long long)q.steps_per_chunk * q.n_chunks <= (long long)INT_MAX, "pixie_mpm_batch_run: scene %d: %d x %d substeps exceed a call",
                   s, q.n_chunks, q.steps_per_chunk);
        PX_REQUIRE(q.n_out >= 0 && q.n_out <= h->S.n, "pixie_mpm_batch_run: scene %d: n_out %d (the scene has %d particles)", s, q.n_out, h->S.n);
        if (q.n_out > 0) {
            PX_REQUIRE(q.d_pos, "pixie_mpm_batch_run: scene %d: n_out %d with a null d_pos", s, q.n_out);
            PX_REQUIRE(std::isfinite(q.scale) && q.scale != 0.0, "pixie_mpm_batch_run: scene %d: bad scale %g", s, q.scale);
        }
        sc[s].dt = q.dt;
        sc[s].chunk = q.steps_per_chunk;
        sc[s].n_chunks = q.n_chunks;
        sc[s].total = q.steps_per_chunk * q.n_chunks;
        sc[s].exp = q.n_out > 0 && q.n_chunks > 0;
        if (sc[s].exp) {
            ex[s].X = make_frame_xform(q.shift, q.scale, q.mean, q.inv_rotation);
            ex[s].init_cov = h->init_cov;
            ex[s].pos = q.d_pos;
            ex[s].cov = q.d_cov;
            ex[s].n_out = q.n_out;
        }
        if (splats && (splats[s].d_log_scale || splats[s].d_quat)) {
            const pixie_batch_splat_out& o = splats[s];
            PX_REQUIRE(o.d_log_scale && o.d_quat, "pixie_mpm_batch_run_splats: scene %d: only one of d_log_scale / d_quat is set", s);
            PX_REQUIRE(q.n_out > 0, "pixie_mpm_batch_run_splats: scene %d: splat outputs with n_out 0 (nothing is exported)", s);
            PX_REQUIRE(q.d_cov, "pixie_mpm_batch_run_splats: scene %d: splat outputs need d_cov (the splats are decomposed covariances)", s);
            spl[s].log_scale = o.d_log_scale;
            spl[s].quat = o.d_quat;
        }
    }
    for (int s = 0; s < ns; ++s)
        if (batch_check_handle(b->h[s], s, "pixie_mpm_batch_run")) return 1;
    int dev = -1;
    PX_CHECK_HIP(hipGetDevice(&dev));
    PX_REQUIRE(dev == b->device, "pixie_mpm_batch_run: HIP device %d is current, the batch was created on device %d", dev, b->device);
    return batch_schedule(b, sc, ex, spl, as_stream(stream));
}

int pixie_mpm_batch_destroy(pixie_mpm_batch* b) {
    if (!b) return 0;
    if (b->finished) (void)hipEventSynchronize(b->finished);
    for (hipEvent_t e : b->ev_up)
        if (e) (void)hipEventSynchronize(e);
    if (b->d_tab) (void)hipFree(b->d_tab);
    for (unsigned char* hb : b->h_buf)
        if (hb) (void)hipHostFree(hb);
    for (hipEvent_t e : b->ev_up)
        if (e) (void)hipEventDestroy(e);
    if (b->finished) (void)hipEventDestroy(b->finished);
    delete b;
    return 0;
}

#ifdef PIXIE_DIAG
int pixie_mpm_phase(pixie_mpm* h, int phase, double dt, void* stream) {
    PX_REQUIRE(h, "null handle");
    hipStream_t st = as_stream(stream);
    const StepParams sp = make_params(h, dt, h->time);
    if (phase == 0) {
        PX_REQUIRE(!h->dirty_grid, "phase 0 called twice without a grid update");
        h->dirty_grid = true;
        return launch_particle(h, false, true, sp, st);
    } else if (phase == 1) {
        h->dirty_grid = false;
        return launch_grid(h, sp, dt, st);
    } else if (phase == 2) {
        return launch_particle(h, true, false, sp, st);
    }
    return set_error("pixie_mpm_phase: unknown phase %d", phase);
}
#endif

int pixie_mpm_export_cov(pixie_mpm* h, float* d_cov, void* stream) {
    PX_REQUIRE(h && d_cov, "null argument");
    hipLaunchKernelGGL(cov_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, h->init_cov, d_cov, h->S.perm);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_export_frame(pixie_mpm* h, int n_out, const double shift[3], double scale, const double mean[3],
                           const double inv_rotation[9], float* d_pos, float* d_cov, void* stream) {
    PX_REQUIRE(h && shift && mean && inv_rotation && d_pos, "pixie_mpm_export_frame: null argument");
    PX_REQUIRE(n_out > 0 && n_out <= h->S.n && scale != 0.0, "pixie_mpm_export_frame: bad n_out / scale");
    const FrameXform X = make_frame_xform(shift, scale, mean, inv_rotation);
    hipLaunchKernelGGL(frame_export_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, h->init_cov, X, n_out, d_pos, d_cov);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_export_frame_splats(pixie_mpm* h, int n_out, const double shift[3], double scale, const double mean[3],
                                  const double inv_rotation[9], float* d_pos, float* d_cov, float* d_log_scale, float* d_quat, void* stream) {
    PX_REQUIRE(h && shift && mean && inv_rotation, "pixie_mpm_export_frame_splats: null argument");
    PX_REQUIRE(n_out > 0 && n_out <= h->S.n && scale != 0.0, "pixie_mpm_export_frame_splats: bad n_out %d / scale %g", n_out, scale);
    PX_REQUIRE(d_pos && d_cov && d_log_scale && d_quat, "pixie_mpm_export_frame_splats: null output (d_pos, d_cov, d_log_scale and d_quat are all required)");
    const FrameXform X = make_frame_xform(shift, scale, mean, inv_rotation);
    hipLaunchKernelGGL(frame_splat_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, h->init_cov, X, n_out, d_pos, d_cov,
                       d_log_scale, d_quat);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_splat_from_cov(const float* d_cov, int64_t n, float* d_log_scale, float* d_quat, void* stream) {
    PX_REQUIRE(n >= 0, "pixie_splat_from_cov: n %lld < 0", (long long)n);
    if (n == 0) return 0;
    PX_REQUIRE(d_cov && d_log_scale && d_quat, "pixie_splat_from_cov: null pointer (d_cov, d_log_scale and d_quat are all required)");
    PX_REQUIRE(n <= (int64_t)INT_MAX * 256, "pixie_splat_from_cov: n %lld exceeds one launch", (long long)n);
    hipLaunchKernelGGL(splat_from_cov_kernel, dim3((unsigned)cdiv(n, 256)), dim3(256), 0, as_stream(stream), d_cov, (long)n, d_log_scale, d_quat);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_export_R(pixie_mpm* h, float* d_R, void* stream) {
    PX_REQUIRE(h && d_R, "null argument");
    hipLaunchKernelGGL(rot_kernel, dim3(cdiv(h->S.n, 256)), dim3(256), 0, as_stream(stream), h->S, d_R, h->S.perm);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_mpm_out_of_bounds(pixie_mpm* h, int64_t* count, void* stream) {
    PX_REQUIRE(h && count, "null argument");
    unsigned long long v[3] = {0, 0, 0};
    PX_CHECK_HIP(hipMemcpyAsync(v, h->S.oob, sizeof v, hipMemcpyDeviceToHost, as_stream(stream)));
    PX_CHECK_HIP(hipStreamSynchronize(as_stream(stream)));
    *count = (int64_t)(v[0] + v[2]);  // left the grid + left every active block (see p2g_scatter_global)
    return 0;
}

#ifdef PIXIE_DIAG
int pixie_mpm_kernel_times(pixie_mpm* h, double* particle_ms, double* grid_ms, int64_t* n_launches) {
    PX_REQUIRE(h && particle_ms && grid_ms && n_launches, "null argument");
    double tp = 0.0, tg = 0.0;
    for (auto& e : h->ev_particle) {
        PX_CHECK_HIP(hipEventSynchronize(e.second));
        float ms = 0.f;
        PX_CHECK_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        tp += ms;
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    for (auto& e : h->ev_grid) {
        PX_CHECK_HIP(hipEventSynchronize(e.second));
        float ms = 0.f;
        PX_CHECK_HIP(hipEventElapsedTime(&ms, e.first, e.second));
        tg += ms;
        (void)hipEventDestroy(e.first); (void)hipEventDestroy(e.second);
    }
    *n_launches = (int64_t)h->ev_particle.size();
    *particle_ms = h->ev_particle.empty() ? 0.0 : tp / (double)h->ev_particle.size();
    *grid_ms = h->ev_grid.empty() ? 0.0 : tg / (double)h->ev_grid.size();
    h->ev_particle.clear();
    h->ev_grid.clear();
    return 0;
}
#endif

}  // extern "C"
