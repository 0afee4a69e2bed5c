// pixie_amd/csrc/mpm_plan.h -- MPM solver: the host's decisions as pure functions (numbers in, numbers out; no HIP).
//
// mpm.hip and mpm_batch_host.h call these and keep the launches, copies, synchronisations and state writes; g++ compiles this
// header alone for tests/test_mpm_plan.py.  The float / double casts of the BC motion and the float compares of the time windows
// are the behaviour (they are what the kernels and the reference do), not style.
#pragma once

#include <algorithm>
#include <cstddef>
#include <vector>

#include "../../include/pixie_hip.h"
#include "mpm_types.h"

namespace pixie {

// ------------------------------------------------------------------ re-binning
// Cadence: the LDS tile tolerates one cell of drift, and the measured drift of the interval just finished
// predicts the next one -- aim at 0.4 cells, never more than four times the last interval (a re-binning of 1 M
// particles costs ~0.4 ms = 4 substeps: with doubling, the ramp 4, 8, ..., 256 of a quiet scene spent six of them in
// the first 252 substeps), and halve when > 0.1 % of the particles were on the slow path.  (The host enqueues substeps
// far ahead of the device, so this is the only feedback.)  The 0.4 is not slack to be spent: aiming at 0.55 / 0.7 cells buys the
// reference's sand configuration 1 / 2 % (9 -> 6 re-binnings in 400 substeps) and costs a 100 k scene in motion 34 % / 183 % -- an
// accelerating scene overshoots the prediction and lands on the slow path (profiles/r6d_drift_target.txt).
// `interval`: the one just finished; `drift_cells`: its largest particle drift; `slow_since`: slow-path particles during it.
inline int next_resort_interval(int interval, double drift_cells, unsigned long long slow_since, int n) {
    int k = interval;
    if (drift_cells > 0.0) k = (int)std::min<double>(4.0 * k, std::max<double>(0.25 * k, k * 0.4 / drift_cells));
    else k = 4 * k;
    if (slow_since > (unsigned long long)n / 1000) k = std::min(k, interval / 2);
    // (ceiling 1024: a re-binning of 1 M particles is ~6 substeps' worth of time, so at 256 it still cost 2.6 % of a
    // quiet scene's run; a scene that wakes up inside a long interval pays through the slow path until the next one)
    return std::max(2, std::min(k, 1024));
}

// Half-size (128-thread) work items iff they would be nearly as few as full-size ones: enter at <= 15 % more, leave above 25 % (a scene
// near the threshold does not flip at every re-binning; the per-item fixed-point scale depends on the item size).
// (Break-even measured near +20 %: 1 M jelly in 200^3, +22 % items, 89.6 vs 90.6 us; the sand configuration, +2 ... 8 % over its
// run, 120 -> 108 us; dense scenes, +64 ... 74 % items, lose 13 %.  profiles/r5e_item_cap_sparse_scenes.txt)
inline bool half_items_wanted(bool half_now, long n128, long n256) {
    return half_now ? n128 * 100 <= n256 * 125 : n128 * 100 <= n256 * 115;
}

// max / min of the positive particle masses as measured by mass_range_kernel; 1 when the measurement is empty or not finite
inline float mass_contrast_of(float lo, float hi) { return (lo > 0.0f && hi >= lo && hi < 3.0e38f) ? hi / lo : 1.0f; }

// Scatter mode (32: packed pairs of 32-bit sums, 64: exact 64-bit fixed point): the caller's, else by the mass contrast
// (see mass_range_kernel for why the packed mode stops at kPackMaxContrast)
constexpr float kPackMaxContrast = 32.0f;
inline int scatter_bits_for(int user, float mass_contrast) { return user ? user : (mass_contrast > kPackMaxContrast ? 64 : 32); }

// ------------------------------------------------------------------ kernel choice
// Which fused G2P + P2G kernel the scene calls for (the variants differ in instruction order, not only in speed: a scene keeps its
// variant in a batched launch too).  Latency-optimised variant (no scheduling barriers, 130 VGPRs = three waves per SIMD = three
// 256-thread work items per CU at once): up to that many the whole work list is resident in one round and a launch lasts one work
// item's latency.  `wide`: -1 auto, 0 / 1 forced.
enum FusedVariant { FV_FIVE_WAVES = 0, FV_WIDE = 1, FV_SIX_WAVES = 2 };
inline FusedVariant fused_variant(int wide, int n_items, int n_cus, int occupancy, int scatter_bits) {
    if (wide == 1 || (wide < 0 && n_items <= 3 * n_cus)) return FV_WIDE;
    if (occupancy >= 6 && scatter_bits != 32) return FV_SIX_WAVES;   // six waves per SIMD: the exact scatter only (the one measured and tested)
    return FV_FIVE_WAVES;
}

// The grid kernel runs one wave per active block.  Its RB = 4 instantiation fits two waves per SIMD: with more active blocks
// than that (1 M particles in 120^3: ~2600 on 2048 slots) the launch takes a second round of waves and the leaner RB = 1
// instantiation + sparse tiles win (14.9 -> 12.5 us); below it (100 k in 50^3: ~520) a launch is one wave's latency and the
// fewer dependent loads the better (whole tiles, RB = 4: 18.7 vs 20.9 us per substep).
// `n_blocks`: a scene's active blocks, or the total of a batched launch.
inline bool grid_crowded(long n_blocks, int n_cus) { return n_blocks > 8L * n_cus; }

// ------------------------------------------------------------------ boundary conditions, modifiers, export transform
inline BCDev to_dev(const pixie_bc_desc& b) {
    BCDev d{};
    d.type = b.type; d.surface_type = b.surface_type; d.reset = b.reset;
    for (int k = 0; k < 3; ++k) {
        d.point[k] = (float)b.point[k]; d.size[k] = (float)b.size[k];
        d.velocity[k] = (float)b.velocity[k]; d.normal[k] = (float)b.normal[k];
    }
    d.start = (float)b.start_time; d.end = (float)b.end_time; d.friction = (float)b.friction;
    return d;
}

// The BCs of one launch, as the kernels take them
inline BCSet make_bcset(const std::vector<BCDev>& bcs_dev, size_t first) {
    BCSet set{};
    set.n = (int)std::min<size_t>(kMaxBCPerLaunch, bcs_dev.size() - std::min(first, bcs_dev.size()));
    for (int k = 0; k < set.n; ++k) set.bc[k] = bcs_dev[first + k];
    return set;
}

// host `modify` of moving cuboids (mpm_solver_warp.py:899-905) after the grid update of the substep at `time`:
// python-float maths, stored as f32
// (on explicit state: pixie_mpm_batch_step runs it ahead on copies to precompute a call's BC table)
inline void advance_bcs_state(double time, std::vector<pixie_bc_desc>& bcs, std::vector<BCDev>& bcs_dev, double dt) {
    for (size_t k = 0; k < bcs.size(); ++k) {
        pixie_bc_desc& b = bcs[k];
        if (b.type != PIXIE_BC_CUBOID) continue;
        const double t0 = (double)(float)b.start_time, t1 = (double)(float)b.end_time;
        if (time >= t0 && time < t1) {
            for (int d = 0; d < 3; ++d) {
                const float np = (float)((double)bcs_dev[k].point[d] + dt * (double)bcs_dev[k].velocity[d]);
                bcs_dev[k].point[d] = np;
                b.point[d] = np;
            }
        }
    }
}

// particle modifiers whose window contains `time` (float compare, as the kernels do), impulses first (mpm_solver_warp.py:529-547);
// `all`: every registered modifier in that order (the batched kernels, where apply_pmod checks the windows)
inline std::vector<PModDev> active_pmods(const std::vector<PModDev>& pmods, float time, bool all = false) {
    std::vector<PModDev> ordered;
    for (int pass = 0; pass < 2; ++pass)
        for (size_t k = 0; k < pmods.size(); ++k) {
            const PModDev& pm = pmods[k];
            if ((pm.type == PIXIE_PM_IMPULSE) != (pass == 0)) continue;
            if (!all && !(time >= pm.start && time < pm.end)) continue;
            ordered.push_back(pm);
        }
    return ordered;
}

// the export transform of pixie_mpm_export_frame / pixie_mpm_batch_run (float conversions of the caller's doubles)
inline FrameXform make_frame_xform(const double shift[3], double scale, const double mean[3], const double inv_rotation[9]) {
    FrameXform X{};
    for (int d = 0; d < 3; ++d) { X.shift[d] = (float)shift[d]; X.mean[d] = (float)mean[d]; }
    X.inv_scale = (float)(1.0 / scale); X.inv_scale2 = (float)(1.0 / (scale * scale));
    for (int c = 0; c < 9; ++c) X.M[c] = (float)inv_rotation[c];
    return X;
}

// ------------------------------------------------------------------ batched launches
// One block-kernel launch per group of scenes that share a kernel variant: the launch kind (g2p, p2g) -- scenes at different points
// of their schedules are fused, G2P-only (a chunk's last substep) or P2G-only (a chunk's first) at the same global step -- the
// work-item capacity (blockDim), when the launch scatters the scatter mode, and for the fused launch each scene's own fused_variant
// (the wide and the five-wave kernels round differently: test_latency_optimised_variant_matches).  The XCD remap does not change bits
// and is chosen for the launch (on when every scene has it on).  Scenes whose plan has `run` unset take no part.
struct BatchSceneKind {
    bool run, g2p, p2g;
    int item_cap;
    bool pack;            // packed 32-bit scatter
    FusedVariant fv;
    int n_items;
    bool xcd_order;
};
struct BatchGroup {
    bool g2p, p2g, pack;  // of the group's first scene: what selects the kernel
    int item_cap;
    FusedVariant fv;
    int n;                     // scenes in the launch
    int xcd_order;
    int scene[kMaxBatch];
    int first[kMaxBatch + 1];  // running sum of the scenes' work items; first[n] = total
    long total;
};
// The next group: led by the first scene that runs and is in no group yet (`done`, one flag per scene, zero before the first call),
// joined by every later one of its kind, in scene order.  false: every running scene has been grouped.
inline bool next_batch_group(const BatchSceneKind* sc, int ns, char* done, BatchGroup* g) {
    int s0 = 0;
    while (s0 < ns && (done[s0] || !sc[s0].run)) ++s0;
    if (s0 == ns) return false;
    const BatchSceneKind& k0 = sc[s0];
    g->g2p = k0.g2p; g->p2g = k0.p2g; g->pack = k0.pack; g->item_cap = k0.item_cap; g->fv = k0.fv;
    g->n = 0;
    g->xcd_order = 1;
    long total = 0;
    for (int s = s0; s < ns; ++s) {
        const BatchSceneKind& k = sc[s];
        if (done[s] || !k.run || k.g2p != k0.g2p || k.p2g != k0.p2g) continue;
        if (k.item_cap != k0.item_cap || (k0.p2g && k.pack != k0.pack)) continue;
        if (k0.g2p && k0.p2g && k.fv != k0.fv) continue;
        done[s] = 1;
        g->scene[g->n] = s;
        g->first[g->n] = (int)total;
        total += k.n_items;
        if (!k.xcd_order) g->xcd_order = 0;
        ++g->n;
    }
    g->first[g->n] = (int)total;
    g->total = total;
    return true;
}

// Byte layout of a window's tables in d_tab / h_tab (batch_upload): the scene descriptors, then 256-aligned each scene's
// StepParams table (n_win + 1 entries, 16-aligned), then each scene's BCSet records (one of `bc_head + n_bc * bc_dev` bytes rounded
// up to 16; one per window step when a cuboid moves, with that stride), then the call's export and splat records, 16-aligned.
struct BatchTableSizes { size_t scene, step_params, bc_head, bc_dev, export_rec, splat_rec; };   // sizeof of the records
struct BatchTableLayout {
    std::vector<size_t> sp_off, bc_off, bc_stride;   // per scene; bc_stride 0: one record for the whole window
    size_t ex_off = 0, spl_off = 0;                  // 0: none
    size_t total = 0;
};
inline size_t align_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
inline void batch_table_layout(const BatchTableSizes& z, int ns, const int* n_win, const size_t* n_bc, const char* moving,
                               bool with_export, bool with_splats, BatchTableLayout* out) {
    out->sp_off.assign(ns, 0); out->bc_off.assign(ns, 0); out->bc_stride.assign(ns, 0);
    size_t off = align_up(z.scene * ns, 256);
    for (int s = 0; s < ns; ++s) {
        out->sp_off[s] = off;
        off = align_up(off + (size_t)(n_win[s] + 1) * z.step_params, 16);
    }
    for (int s = 0; s < ns; ++s) {
        const size_t rec = align_up(z.bc_head + n_bc[s] * z.bc_dev, 16);
        out->bc_stride[s] = moving[s] ? rec : 0;
        out->bc_off[s] = off;
        off += moving[s] ? rec * (size_t)n_win[s] : rec;
    }
    out->ex_off = 0;
    if (with_export) {
        out->ex_off = off = align_up(off, 16);
        off += (size_t)ns * z.export_rec;
    }
    out->spl_off = 0;
    if (with_splats) {
        out->spl_off = off = align_up(off, 16);
        off += (size_t)ns * z.splat_rec;
    }
    out->total = off;
}

}  // namespace pixie
