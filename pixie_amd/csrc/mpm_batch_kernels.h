// pixie_amd/csrc/mpm_batch_kernels.h -- MPM device code: several scenes per launch (pixie_mpm_batch_*).
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// ------------------------------------------------------------------ several scenes per launch (pixie_mpm_batch_*)
// A 100 k-particle scene gives one launch ~500 work items and ~2000 active blocks: too little to fill the chip, and each scene pays
// its own two launches per substep.  The batched wrappers put the work items of up to kMaxBatch scenes into ONE block-kernel launch
// and their active blocks into ONE grid-kernel launch, then run the solo kernels' own bodies on them.
//
// Where the per-scene parameters come from (kernel arguments would be ~2 KB per scene, and a copy per launch costs about what the
// launch saves):
//   * BatchScene, one per scene, in device memory: the scene's MpmPtrs, ALL its registered modifiers (impulses first -- the order of
//     active_pmods; apply_pmod re-checks each window with the same float compare, so applying the inactive ones is a no-op), and
//     pointers into this call's tables.  Written at the start of each pixie_mpm_batch_step and again after a re-binning of the scene
//     (rebin() has just synchronised the stream: nothing in flight reads the old descriptor).
//   * this call's tables, precomputed on the host at the start of the call and uploaded with the descriptors in ONE copy: the
//     StepParams of every substep (only `time` advances) and the BCSet of every grid launch (moving cuboids advance in double on the
//     host and are stored as float, advance_bcs_state) -- one BCSet for the whole call when the scene has no cuboid.
//   * BatchLaunch, the kernel argument (~270 bytes): which scenes this launch covers and the prefix of their work items (or active
//     blocks).  Everything that changes at a re-binning of one scene -- item counts, the capacity that groups launches -- is here.
// The descriptor is read through an address-space-4 (constant) pointer with a wave-uniform scene index: scalar loads, as the solo
// kernels' parameters are.  The block kernel copies MpmPtrs and StepParams into locals at entry: read through references the same
// body was scheduled differently from the solo kernel and contracted other multiply-adds (F_trial differed in the last bit).
struct BatchScene {
    MpmPtrs S;
    PModSet pms;                   // every registered modifier, impulses first
    const StepParams* sp;          // [n_substeps + 1] of this call: the launch of `step` reads sp[step]
    const unsigned char* bcs;      // BCSet records of this call's grid launches: grid launch `step` reads bcs + step * bc_stride
    long long bc_stride;           // 0: no cuboid -- one record for the whole call
};
struct BatchLaunch {
    const BatchScene* scenes;      // device descriptors
    int n;                         // scenes in this launch
    int step;                      // substep index into the call's tables
    int xcd_order;                 // work items dealt to the XCDs in contiguous runs (as mpm_block_kernel)
    int pad;
    int scene[kMaxBatch];          // descriptor of launch scene k
    int first[kMaxBatch + 1];      // first global work item (block kernel) / active block (grid kernel) of launch scene k
};
typedef const BatchScene __attribute__((address_space(4))) ConstBatchScene;

// launch scene of global index `g` (wave-uniform: g is a workgroup index), and the descriptor it reads
// (Launch: BatchLaunch, or ExportLaunch of the batched frame export)
template <class Launch>
__device__ __forceinline__ int batch_scene_of(const Launch& L, int g) {
    int k = 0;
    for (int j = 1; j < L.n; ++j) k += (g >= L.first[j]) ? 1 : 0;
    return __builtin_amdgcn_readfirstlane(k);
}
// what a descriptor points at (this call's tables) is read the same way: through a constant-address-space view of the pointer
template <class T>
__device__ __forceinline__ const T& const_view(const T* p) {
    return *(const T*)(const T __attribute__((address_space(4)))*)p;
}
template <class Launch>
__device__ __forceinline__ const BatchScene& batch_desc(const Launch& L, int k) {
    const ConstBatchScene* d = (const ConstBatchScene*)L.scenes + L.scene[k];
    return *(const BatchScene*)d;
}

template <bool DO_G2P, bool DO_P2G, int OCC, int FL>
__global__ __launch_bounds__(kWG, OCC) void mpm_block_batch_kernel(BatchLaunch BL) {
    constexpr bool PACK = (FL & F_PACK32) != 0;     // (the prologue of mpm_block_kernel)
    constexpr bool TRACE = (FL & F_TRACE) != 0;
    constexpr bool SCHED = (FL & F_WIDE) == 0;
    __shared__ float4 tv[kTN];
    __shared__ unsigned long long ta[PACK ? 2 : 4][kTN];
    __shared__ float s_red[2][kWG / 64];
    // global work item (remapped over the XCDs like mpm_block_kernel's) -> (scene, the scene's own work item)
    int item = (int)blockIdx.x;
    if (BL.xcd_order) {
        const int per = (int)gridDim.x >> 3;
        if (item < (per << 3)) item = (item & 7) * per + (item >> 3);
    }
    const int k = batch_scene_of(BL, item);
    const BatchScene& D = batch_desc(BL, k);
    const MpmPtrs S = D.S;
    const StepParams sp = const_view(D.sp + BL.step);
    const PModSet& pms = D.pms;
    item -= BL.first[k];
#include "mpm_block_body.h"
}

template <int RB>
__global__ __launch_bounds__(64) void mpm_grid_block_batch_kernel(BatchLaunch L) {
    const int slot = (int)blockIdx.x;
    const int k = batch_scene_of(L, slot);
    const BatchScene& D = batch_desc(L, k);
    const BCSet& bcs = const_view(reinterpret_cast<const BCSet*>(D.bcs + (size_t)L.step * (size_t)D.bc_stride));
    grid_block_update<RB>(D.S, const_view(D.sp + L.step), bcs, slot - L.first[k], D.S.gout);
}

}  // namespace pixie
