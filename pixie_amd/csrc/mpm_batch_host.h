// pixie_amd/csrc/mpm_batch_host.h -- MPM solver, host side of pixie_mpm_batch_*: the table upload, the grouped launches and the
// schedule of one call.  Part of the mpm.hip translation unit (included after the solo handle's plan / issue functions).
#pragma once

// Several scenes stepped with one block-kernel and one grid-kernel launch per substep (see BatchScene for the device side).
struct pixie_mpm_batch {
    std::vector<pixie_mpm*> h;
    std::vector<MpmPtrs> desc_S;             // each scene's MpmPtrs as last uploaded (byte copies: compared with memcmp)
    unsigned char* d_tab = nullptr;          // descriptors, then this call's StepParams tables and BCSet records
    unsigned char* h_tab = nullptr;          // pinned staging image of d_tab for the current call: h_buf[cur_buf]
    unsigned char* h_buf[2] = {nullptr, nullptr};   // two, used by alternate calls: a call waits only for the copies of the call before last
    size_t cap = 0;
    std::vector<size_t> sp_off;              // this window's StepParams table of scene s, in d_tab / h_tab
    size_t ex_off = 0;                       // this call's export records (BatchExport per scene), if it exports
    size_t spl_off = 0;                      // this call's splat records (BatchSplat per scene), if a scene exports splats
    hipEvent_t ev_up[2] = {nullptr, nullptr};      // after the last copy out of h_buf[i] (h_buf[i] is rewritten only once it has run)
    int cur_buf = 1;
    int device = 0;                          // the HIP device current at creation: the events and tables live there
    hipEvent_t finished = nullptr;           // after the last launch of the last call (d_tab is freed / reallocated only then)
    int n_cus = 256;
};

namespace {

// what a batched step does not cover (the fallbacks of launch_grid / launch_particle, the diagnostic kernels); checked before
// anything is launched or changed
int batch_check_handle(const pixie_mpm* h, int s, const char* what) {
    PX_REQUIRE(!h->dirty_grid, "%s: scene %d has a phase-API P2G pending", what, s);
    PX_REQUIRE(h->trace == 0, "%s: scene %d has `trace` set (the diagnostic kernels are not batched)", what, s);
    PX_REQUIRE(h->bcs_dev.size() <= (size_t)kMaxBCPerLaunch, "%s: scene %d has %zu boundary conditions; a batched step takes at most %d per scene",
               what, s, h->bcs_dev.size(), kMaxBCPerLaunch);
    PX_REQUIRE(h->pmods.size() <= (size_t)kMaxPModFused, "%s: scene %d has %zu particle modifiers; a batched step takes at most %d per scene",
               what, s, h->pmods.size(), kMaxPModFused);
    return 0;
}

// One call's schedule for one scene (pixie_mpm_batch_run, validated): n_chunks chunks of `chunk` substeps of dt, the scene's
// substep j being the call's global step j; `exp`: a frame export before every chunk (BatchExport record).
struct BatchSched {
    double dt = 0.0;
    int chunk = 0;
    int n_chunks = 0;
    int total = 0;                 // chunk * n_chunks
    bool exp = false;
};

// Long calls are tabled in windows of kBatchWindow global steps: a moving cuboid stores one BCSet record (up to ~1.4 KB) per substep,
// and a 200-frame metal scene is 200 000 substeps.
constexpr int kBatchWindow = 1024;

// Start of a window [g0, g0 + kBatchWindow) of a call: the descriptors and the window's tables -- per scene, the StepParams of global
// steps g0 ... g0 + n and the BCSet of grid launches g0 ... g0 + n - 1, n = the scene's substeps in the window -- are computed on the
// host by running the solo step's own time / BC bookkeeping (make_params, make_bcset, advance_bcs_state) ahead on copies of the
// handle's state, which the plans of the steps before g0 have brought to global step g0, and uploaded in one copy.  Launches index
// the tables with the step relative to g0.  The plan of every substep checks what it computes against these tables (batch_expect_*).
// `ex`: the call's export records, uploaded with every window (NULL: the call does not export); `spl` likewise its splat records
// (NULL: no scene exports splats).
int batch_upload(pixie_mpm_batch* b, const std::vector<BatchSched>& sc, int g0, const std::vector<BatchExport>* ex,
                 const std::vector<BatchSplat>* spl, hipStream_t st) {
    const int ns = (int)b->h.size();
    std::vector<int> n_win(ns);
    std::vector<size_t> n_bc(ns);
    std::vector<char> moving(ns, 0);
    for (int s = 0; s < ns; ++s) {
        const pixie_mpm* h = b->h[s];
        n_win[s] = std::max(0, std::min(sc[s].total - g0, kBatchWindow));
        n_bc[s] = h->bcs_dev.size();
        for (const pixie_bc_desc& bc : h->bcs) moving[s] = moving[s] || bc.type == PIXIE_BC_CUBOID;
    }
    const size_t head = offsetof(BCSet, bc);
    const BatchTableSizes sizes{sizeof(BatchScene), sizeof(StepParams), head, sizeof(BCDev), sizeof(BatchExport), sizeof(BatchSplat)};
    BatchTableLayout lay;
    batch_table_layout(sizes, ns, n_win.data(), n_bc.data(), moving.data(), ex != nullptr, spl != nullptr, &lay);
    const std::vector<size_t>& bc_off = lay.bc_off;
    const std::vector<size_t>& bc_stride = lay.bc_stride;
    const size_t off = lay.total, ex_off = lay.ex_off, spl_off = lay.spl_off;
    b->sp_off = lay.sp_off;
    // Rewriting d_tab between the windows of a call is safe without a synchronisation: the copy below is issued on `st`, the stream
    // of every launch of the call, after the last launch of the previous window, and a launch of this window is issued after it.
    // (The staging buffer is another matter: h_buf[cur_buf] is rewritten only once ev_up says its last copy has run.)
    b->cur_buf ^= 1;
    PX_CHECK_HIP(hipEventSynchronize(b->ev_up[b->cur_buf]));   // the copies of the window before last (a no-op for an event never recorded)
    if (off > b->cap) {
        // launches of the last call may still read d_tab, and its copies may still read the other staging buffer.  (Within a call
        // the first window is the largest -- scenes only drop out -- so this runs at g0 == 0; the stream synchronisation covers the
        // call's own earlier launches otherwise.)
        PX_CHECK_HIP(hipEventSynchronize(b->finished));
        if (g0 > 0) PX_CHECK_HIP(hipStreamSynchronize(st));
        PX_CHECK_HIP(hipEventSynchronize(b->ev_up[b->cur_buf ^ 1]));
        if (b->d_tab) (void)hipFree(b->d_tab);
        for (unsigned char*& hb : b->h_buf) { if (hb) (void)hipHostFree(hb); hb = nullptr; }
        b->d_tab = nullptr; b->cap = 0;
        const size_t cap = align_up(off + off / 2, 4096);
        PX_CHECK_HIP(hipMalloc((void**)&b->d_tab, cap));
        for (unsigned char*& hb : b->h_buf) PX_CHECK_HIP(hipHostMalloc((void**)&hb, cap));
        b->cap = cap;
    }
    b->h_tab = b->h_buf[b->cur_buf];
    b->desc_S.resize(ns);
    for (int s = 0; s < ns; ++s) {
        pixie_mpm* h = b->h[s];
        BatchScene D;
        memset(&D, 0, sizeof D);
        memcpy(&D.S, &h->S, sizeof(MpmPtrs));
        memcpy(&b->desc_S[s], &h->S, sizeof(MpmPtrs));
        const std::vector<PModDev> all = active_pmods(h->pmods, 0.0f, true);
        D.pms.n = (int)all.size();
        for (int k = 0; k < D.pms.n; ++k) D.pms.pm[k] = all[k];
        D.sp = reinterpret_cast<const StepParams*>(b->d_tab + b->sp_off[s]);
        D.bcs = b->d_tab + bc_off[s];
        D.bc_stride = (long long)bc_stride[s];
        memcpy(b->h_tab + s * sizeof(BatchScene), &D, sizeof D);
        const double dt = sc[s].dt;
        double t = h->time;
        std::vector<pixie_bc_desc> bcs = h->bcs;
        std::vector<BCDev> bcs_dev = h->bcs_dev;
        StepParams* spt = reinterpret_cast<StepParams*>(b->h_tab + b->sp_off[s]);
        spt[0] = make_params(h, dt, t);
        for (int i = 0; i < n_win[s]; ++i) {    // the order of pixie_mpm_step: grid launch at t, `modify`, t += dt, G2P/P2G at t
            if (bc_stride[s] || i == 0) {
                const BCSet set = make_bcset(bcs_dev, 0);
                memcpy(b->h_tab + bc_off[s] + (size_t)i * bc_stride[s], &set, head + (size_t)set.n * sizeof(BCDev));
            }
            advance_bcs_state(t, bcs, bcs_dev, dt);
            t = t + dt;
            spt[i + 1] = make_params(h, dt, t);
        }
    }
    b->ex_off = ex_off;
    if (ex) memcpy(b->h_tab + ex_off, ex->data(), (size_t)ns * sizeof(BatchExport));
    b->spl_off = spl_off;
    if (spl) memcpy(b->h_tab + spl_off, spl->data(), (size_t)ns * sizeof(BatchSplat));
    PX_CHECK_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, off, hipMemcpyHostToDevice, st));
    PX_CHECK_HIP(hipEventRecord(b->ev_up[b->cur_buf], st));
    return 0;
}

int batch_expect_sp(const pixie_mpm_batch* b, int s, int step, const StepParams& sp) {
    const StepParams* spt = reinterpret_cast<const StepParams*>(b->h_tab + b->sp_off[s]);
    PX_REQUIRE(memcmp(&spt[step], &sp, sizeof sp) == 0, "pixie_mpm_batch: scene %d: parameters of window step %d differ from the call's table (internal error)", s, step);
    return 0;
}
int batch_expect_bcs(const pixie_mpm_batch* b, int s, int step, const BCSet& set) {
    const BatchScene* D = reinterpret_cast<const BatchScene*>(b->h_tab) + s;
    const unsigned char* rec = b->h_tab + (D->bcs - b->d_tab) + (size_t)step * (size_t)D->bc_stride;
    PX_REQUIRE(memcmp(rec, &set, offsetof(BCSet, bc) + (size_t)set.n * sizeof(BCDev)) == 0,
               "pixie_mpm_batch: scene %d: BCs of window step %d differ from the call's table (internal error)", s, step);
    return 0;
}

// After the plan of a launch: a scene whose MpmPtrs changed (a re-binning: new row copy, sparse-tile mode) gets its descriptor
// rewritten.  rebin() ends with a stream synchronisation, so nothing in flight reads the descriptors or copies out of h_tab;
// the synchronisation below is that guarantee made explicit and costs nothing then.
int batch_refresh(pixie_mpm_batch* b, hipStream_t st) {
    const int ns = (int)b->h.size();
    bool changed = false;
    for (int s = 0; s < ns; ++s) changed = changed || memcmp(&b->desc_S[s], &b->h[s]->S, sizeof(MpmPtrs)) != 0;
    if (!changed) return 0;
    PX_CHECK_HIP(hipStreamSynchronize(st));
    for (int s = 0; s < ns; ++s) {
        memcpy(&b->desc_S[s], &b->h[s]->S, sizeof(MpmPtrs));
        memcpy(b->h_tab + s * sizeof(BatchScene) + offsetof(BatchScene, S), &b->h[s]->S, sizeof(MpmPtrs));
    }
    PX_CHECK_HIP(hipMemcpyAsync(b->d_tab, b->h_tab, (size_t)ns * sizeof(BatchScene), hipMemcpyHostToDevice, st));
    PX_CHECK_HIP(hipEventRecord(b->ev_up[b->cur_buf], st));
    return 0;
}

struct BatchBlockLaunch {
    static constexpr bool kHasTrace = false;   // batch_check_handle refuses scenes with `trace` set
    const BatchLaunch& L;
    unsigned n_wg;
    int cap;
    hipStream_t st;
    template <bool G, bool P, int OCC, int FL>
    void run() const {
        hipLaunchKernelGGL((mpm_block_batch_kernel<G, P, OCC, FL>), dim3(n_wg), dim3((unsigned)cap), 0, st, L);
    }
};

// One block-kernel launch per group of scenes that share a kernel variant (next_batch_group says which do), in the variant that
// dispatch_block_variant gives the group's first scene.
int batch_issue_particle(pixie_mpm_batch* b, const std::vector<ParticlePlan>& pl, int step, hipStream_t st) {
    const int ns = (int)b->h.size();
    BatchSceneKind kind[kMaxBatch];
    char done[kMaxBatch] = {};
    for (int s = 0; s < ns; ++s) {
        const pixie_mpm* h = b->h[s];
        kind[s] = BatchSceneKind{pl[s].run, pl[s].g2p, pl[s].p2g, h->item_cap, h->scatter_bits == 32, fused_variant(h), h->n_items, h->xcd_order != 0};
    }
    BatchGroup g;
    while (next_batch_group(kind, ns, done, &g)) {
        PX_REQUIRE(g.total < (long)INT_MAX, "pixie_mpm_batch_step: %ld work items in one launch", g.total);
        BatchLaunch L;
        memset(&L, 0, sizeof L);
        L.scenes = reinterpret_cast<const BatchScene*>(b->d_tab);
        L.step = step;
        L.xcd_order = g.xcd_order;
        L.n = g.n;
        memcpy(L.scene, g.scene, sizeof(int) * g.n);
        memcpy(L.first, g.first, sizeof(int) * (g.n + 1));
        dispatch_block_variant(g.g2p, g.p2g, g.fv, g.pack, false, BatchBlockLaunch{L, (unsigned)g.total, g.item_cap, st});
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// One grid-kernel launch for every scene whose plan is the plain active-block update (every scene, given batch_check_handle: a
// scene with staged tiles and <= kMaxBCPerLaunch BCs); anything else is issued as the solo step would.  RB from the launch's total.
// Scenes with `on[s]` unset have no substep at this global step and take no part.
int batch_issue_grid(pixie_mpm_batch* b, const std::vector<GridPlan>& gp, const std::vector<char>& on, int step, hipStream_t st) {
    const int ns = (int)b->h.size();
    BatchLaunch L;
    memset(&L, 0, sizeof L);
    L.scenes = reinterpret_cast<const BatchScene*>(b->d_tab);
    L.step = step;
    long total = 0;
    for (int s = 0; s < ns; ++s) {
        if (!on[s]) continue;
        if (!gp[s].single_block_update()) {
            if (issue_grid(b->h[s], gp[s], st)) return 1;
            continue;
        }
        if (batch_expect_bcs(b, s, step, gp[s].ops[0].set)) return 1;
        L.scene[L.n] = s;
        L.first[L.n] = (int)total;
        total += gp[s].ops[0].n_wg;
        ++L.n;
    }
    if (L.n == 0) return 0;
    PX_REQUIRE(total < (long)INT_MAX, "pixie_mpm_batch_step: %ld active blocks in one launch", total);
    L.first[L.n] = (int)total;
    const dim3 g((unsigned)total), blk(64);
    if (grid_crowded(total, b->n_cus)) hipLaunchKernelGGL(mpm_grid_block_batch_kernel<1>, g, blk, 0, st, L);
    else hipLaunchKernelGGL(mpm_grid_block_batch_kernel<4>, g, blk, 0, st, L);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

// One frame_export_batch_kernel launch for every scene with frame[s] >= 0 (the frame it exports) and no splats, and one
// frame_splat_batch_kernel launch for those with splats (splat[s]; empty: none has); none for an empty list.
int batch_issue_export(pixie_mpm_batch* b, const std::vector<int>& frame, const std::vector<char>& splat, hipStream_t st) {
    const int ns = (int)b->h.size();
    for (int with_splat = 0; with_splat < (splat.empty() ? 1 : 2); ++with_splat) {
        ExportLaunch L;
        memset(&L, 0, sizeof L);
        L.scenes = reinterpret_cast<const BatchScene*>(b->d_tab);
        L.ex = reinterpret_cast<const BatchExport*>(b->d_tab + b->ex_off);
        long total = 0;
        for (int s = 0; s < ns; ++s) {
            if (frame[s] < 0 || (!splat.empty() && (splat[s] != 0) != (with_splat != 0))) continue;
            L.scene[L.n] = s;
            L.frame[L.n] = frame[s];
            L.first[L.n] = (int)total;
            total += cdiv(b->h[s]->S.n, 256);
            ++L.n;
        }
        if (L.n == 0) continue;
        L.first[L.n] = (int)total;
        if (with_splat)
            hipLaunchKernelGGL(frame_splat_batch_kernel, dim3((unsigned)total), dim3(256), 0, st, L,
                               reinterpret_cast<const BatchSplat*>(b->d_tab + b->spl_off));
        else
            hipLaunchKernelGGL(frame_export_batch_kernel, dim3((unsigned)total), dim3(256), 0, st, L);
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

// The launches of one call.  Every scene runs its chunks with the launch sequence of pixie_mpm_step -- a P2G-only launch, then per
// substep [grid launch at t, t += dt, fused G2P + P2G, or G2P-only on the chunk's last substep] -- and its substep j is the call's
// global step j, so the scenes that still have substeps share each global step's grid launch and particle launches (one per
// variant group).  A scene that ends a chunk at a global step and has another one exports its next frame after that step's particle
// launches -- its G2P-only launch has left v / C / F_trial valid (the note on skip_vcft); no export is ever issued inside a chunk,
// frame_export reads F_trial -- and then plans and issues its next chunk's P2G-only launch, so that it joins the next grid launch.
// Frame 0's export precedes everything.  Chunk boundaries are kept as given: each scene sees exactly the pixie_mpm_step calls
// (and exports) of its solo loop, in the same order, on its own host state.
// `spl`: per scene, where its splats go (BatchSplat, NULL pointers: none); empty when no scene exports splats.
int batch_schedule(pixie_mpm_batch* b, const std::vector<BatchSched>& sc, const std::vector<BatchExport>& ex,
                   const std::vector<BatchSplat>& spl, hipStream_t st) {
    const int ns = (int)b->h.size();
    int G = 0;
    bool any_ex = false;
    for (const BatchSched& q : sc) { G = std::max(G, q.total); any_ex = any_ex || q.exp; }
    if (G == 0 && !any_ex) return 0;
    const std::vector<BatchExport>* exr = any_ex ? &ex : nullptr;
    std::vector<char> splat;               // which exporting scenes go through frame_splat_batch_kernel (empty: none)
    for (int s = 0; s < (int)spl.size(); ++s)
        if (sc[s].exp && spl[s].log_scale) { splat.assign(ns, 0); break; }
    for (int s = 0; s < (int)splat.size(); ++s) splat[s] = sc[s].exp && spl[s].log_scale;
    const std::vector<BatchSplat>* splr = splat.empty() ? nullptr : &spl;
    int g0 = 0;
    if (batch_upload(b, sc, g0, exr, splr, st)) return 1;
    std::vector<ParticlePlan> pp(ns);
    std::vector<GridPlan> gp(ns);
    std::vector<char> on(ns, 0), next(ns, 0);
    std::vector<int> frame(ns, -1);
    // frame 0 of every exporting scene (a scene whose chunks are empty exports all its frames here, one launch per frame)
    for (int f = 0; any_ex; ++f) {
        bool any = false;
        for (int s = 0; s < ns; ++s) {
            const bool e = sc[s].exp && f < sc[s].n_chunks && (f == 0 || sc[s].chunk == 0);
            frame[s] = e ? f : -1;
            any = any || e;
        }
        if (!any) break;
        if (batch_issue_export(b, frame, splat, st)) return 1;
    }
    // substep 0 of the first chunk: modifiers + stress + P2G at time t0
    for (int s = 0; s < ns; ++s) {
        pp[s].run = false;
        if (sc[s].total == 0) continue;
        pixie_mpm* h = b->h[s];
        const StepParams sp = make_params(h, sc[s].dt, h->time);
        if (batch_expect_sp(b, s, 0, sp) || plan_particle(h, false, true, sp, st, pp[s])) return 1;
    }
    if (batch_refresh(b, st) || batch_issue_particle(b, pp, 0, st)) return 1;
    for (int g = 0; g < G; ++g) {
        if (g - g0 == kBatchWindow) {
            g0 = g;
            if (batch_upload(b, sc, g0, exr, splr, st)) return 1;
        }
        const int i = g - g0;
        for (int s = 0; s < ns; ++s) {
            on[s] = g < sc[s].total;
            if (!on[s]) continue;
            pixie_mpm* h = b->h[s];
            const StepParams sp = make_params(h, sc[s].dt, h->time);
            if (batch_expect_sp(b, s, i, sp) || plan_grid(h, sp, sc[s].dt, gp[s])) return 1;
        }
        if (batch_issue_grid(b, gp, on, i, st)) return 1;
        bool any_next = false;
        for (int s = 0; s < ns; ++s) {
            pp[s].run = false;
            next[s] = 0;
            frame[s] = -1;
            if (!on[s]) continue;
            pixie_mpm* h = b->h[s];
            h->time = h->time + sc[s].dt;  // mpm_solver_warp.py:637
            const bool last = (g + 1) % sc[s].chunk == 0;
            const StepParams sp = make_params(h, sc[s].dt, h->time);
            if (batch_expect_sp(b, s, i + 1, sp) || plan_particle(h, true, !last, sp, st, pp[s])) return 1;
            if (last && g + 1 < sc[s].total) {
                next[s] = 1;
                any_next = true;
                if (sc[s].exp) frame[s] = (g + 1) / sc[s].chunk;
            }
        }
        if (batch_refresh(b, st) || batch_issue_particle(b, pp, i + 1, st)) return 1;
        if (!any_next) continue;
        // scenes between two chunks: the next frame's export, then the next chunk's P2G-only launch at the same time
        if (batch_issue_export(b, frame, splat, st)) return 1;
        for (int s = 0; s < ns; ++s) {
            pp[s].run = false;
            if (!next[s]) continue;
            pixie_mpm* h = b->h[s];
            const StepParams sp = make_params(h, sc[s].dt, h->time);
            if (batch_expect_sp(b, s, i + 1, sp) || plan_particle(h, false, true, sp, st, pp[s])) return 1;
        }
        if (batch_refresh(b, st) || batch_issue_particle(b, pp, i + 1, st)) return 1;
    }
    PX_CHECK_HIP(hipEventRecord(b->finished, st));
    return 0;
}

}  // namespace
