// pixie_amd/csrc/mpm_export_kernels.h -- MPM device code: covariance, frame, splat, rotation, stress and grid export kernels.
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

__global__ void cov_kernel(MpmPtrs S, const float* __restrict__ init_cov, float* __restrict__ cov, const int* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const int s = perm ? perm[i] : i;
    Mat3 F, M;
    for (int c = 0; c < 9; ++c) F.m[c] = S.Ft[(size_t)c * S.n + i];
    const float* c6 = init_cov + (size_t)s * 6;
    M.m[0] = c6[0]; M.m[1] = c6[1]; M.m[2] = c6[2];
    M.m[3] = c6[1]; M.m[4] = c6[3]; M.m[5] = c6[4];
    M.m[6] = c6[2]; M.m[7] = c6[4]; M.m[8] = c6[5];
    const Mat3 T = mat_mul_bt(mat_mul(F, M), F);
    float* o = cov + (size_t)s * 6;
    o[0] = T.m[0]; o[1] = T.m[1]; o[2] = T.m[2]; o[3] = T.m[4]; o[4] = T.m[5]; o[5] = T.m[8];
}
// Per-frame export for the rasteriser (PG/gs_simulation.py:591-600): positions and covariances of the first n_out
// particles (caller order) in the original scene frame,
//   pos_render = apply_inverse_rotations(undotransform2origin(undoshift2center111(x, z_shift), scale, mean), Rs)
//   cov_render = apply_inverse_cov_rotations(compute_cov_from_F(F_trial, init_cov) / scale^2, Rs)
// (PG/utils/transformation_utils.py:19-20,108-130; compute_cov_from_F mpm_utils.py:529-553) with the rotation chain
// folded into one matrix M on the host: pos @ M, M^T cov M.  The body is shared textually with frame_export_batch_kernel.
__global__ void frame_export_kernel(MpmPtrs S, const float* __restrict__ init_cov, FrameXform X, int n_out, float* __restrict__ pos_out,
                                    float* __restrict__ cov_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#include "frame_export_body.h"
}
// The same export for several scenes of a pixie_mpm_batch in one launch (pixie_mpm_batch_run): one record per scene in the call's
// table (BatchExport), and a launch argument that says which scenes export which frame.  Block b of the launch belongs to launch
// scene k with first[k] <= b < first[k + 1] (ceil(n / 256) blocks per scene, as frame_export_kernel's grid).
struct BatchExport {
    FrameXform X;
    const float* init_cov;
    float* pos;                    // frame 0 of [n_frames][n_out][3]
    float* cov;                    // frame 0 of [n_frames][n_out][6], or NULL
    int n_out;
    int pad;
};
struct ExportLaunch {
    const BatchScene* scenes;      // device descriptors (MpmPtrs kept current by batch_refresh)
    const BatchExport* ex;         // export record of descriptor s: ex[s]
    int n;                         // scenes in this launch
    int pad;
    int scene[kMaxBatch];          // descriptor of launch scene k
    int frame[kMaxBatch];          // the frame launch scene k exports
    int first[kMaxBatch + 1];      // first block of launch scene k
};
__global__ void frame_export_batch_kernel(ExportLaunch L) {
    const int k = batch_scene_of(L, (int)blockIdx.x);
    // (copied into locals first, as mpm_block_batch_kernel does: the body must see what frame_export_kernel's arguments give it)
    const MpmPtrs S = batch_desc(L, k).S;
    const BatchExport E = const_view(L.ex + L.scene[k]);
    const FrameXform X = E.X;
    const float* __restrict__ init_cov = E.init_cov;
    const int n_out = E.n_out;
    float* __restrict__ pos_out = E.pos + (size_t)L.frame[k] * (size_t)n_out * 3;
    float* __restrict__ cov_out = E.cov ? E.cov + (size_t)L.frame[k] * (size_t)n_out * 6 : nullptr;
    const int i = ((int)blockIdx.x - L.first[k]) * 256 + (int)threadIdx.x;
#include "frame_export_body.h"
}
// The frame export with the 3DGS splat parameters of every exported covariance (PG/gs_simulation.py:290-322, the per-frame PLY):
// frame_export_kernel's body, then splat::splat_from_cov of the covariance it has just stored (Rr, the values written to cov_out),
// so the splats are the bits pixie_splat_from_cov gives for that cov.  Needs cov_out (the host refuses NULL).
__global__ void frame_splat_kernel(MpmPtrs S, const float* __restrict__ init_cov, FrameXform X, int n_out, float* __restrict__ pos_out,
                                   float* __restrict__ cov_out, float* __restrict__ log_scale_out, float* __restrict__ quat_out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
#include "frame_export_body.h"
    const float cs[6] = {Rr.m[0], Rr.m[1], Rr.m[2], Rr.m[4], Rr.m[5], Rr.m[8]};
    float ls[3], qt[4];
    splat::splat_from_cov(cs, ls, qt);
    for (int d = 0; d < 3; ++d) log_scale_out[(size_t)s * 3 + d] = ls[d];
    for (int d = 0; d < 4; ++d) quat_out[(size_t)s * 4 + d] = qt[d];
}
// Splat outputs of one scene in a pixie_mpm_batch_run_splats call: a record array of its own in the call's table, beside the
// BatchExport records (indexed alike: descriptor s -> sp[s]).
struct BatchSplat {
    float* log_scale;              // frame 0 of [n_frames][n_out][3]
    float* quat;                   // frame 0 of [n_frames][n_out][4]
};
// frame_export_batch_kernel's twin for the scenes that export splats (the same ExportLaunch, listing only those scenes)
__global__ void frame_splat_batch_kernel(ExportLaunch L, const BatchSplat* __restrict__ sp) {
    const int k = batch_scene_of(L, (int)blockIdx.x);
    const MpmPtrs S = batch_desc(L, k).S;
    const BatchExport E = const_view(L.ex + L.scene[k]);
    const BatchSplat P = const_view(sp + L.scene[k]);
    const FrameXform X = E.X;
    const float* __restrict__ init_cov = E.init_cov;
    const int n_out = E.n_out;
    float* __restrict__ pos_out = E.pos + (size_t)L.frame[k] * (size_t)n_out * 3;
    float* __restrict__ cov_out = E.cov + (size_t)L.frame[k] * (size_t)n_out * 6;
    float* __restrict__ log_scale_out = P.log_scale + (size_t)L.frame[k] * (size_t)n_out * 3;
    float* __restrict__ quat_out = P.quat + (size_t)L.frame[k] * (size_t)n_out * 4;
    const int i = ((int)blockIdx.x - L.first[k]) * 256 + (int)threadIdx.x;
#include "frame_export_body.h"
    const float cs[6] = {Rr.m[0], Rr.m[1], Rr.m[2], Rr.m[4], Rr.m[5], Rr.m[8]};
    float ls[3], qt[4];
    splat::splat_from_cov(cs, ls, qt);
    for (int d = 0; d < 3; ++d) log_scale_out[(size_t)s * 3 + d] = ls[d];
    for (int d = 0; d < 4; ++d) quat_out[(size_t)s * 4 + d] = qt[d];
}
// cov3D_to_log_scales_and_quats (PG/gs_simulation.py:253-288) on its own: [n][6] -> [n][3], [n][4] (wxyz)
__global__ void splat_from_cov_kernel(const float* __restrict__ cov, long n, float* __restrict__ log_scale_out, float* __restrict__ quat_out) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float cs[6];
    for (int d = 0; d < 6; ++d) cs[d] = cov[i * 6 + d];
    float ls[3], qt[4];
    splat::splat_from_cov(cs, ls, qt);
    for (int d = 0; d < 3; ++d) log_scale_out[i * 3 + d] = ls[d];
    for (int d = 0; d < 4; ++d) quat_out[i * 4 + d] = qt[d];
}
// compute_R_from_F, mpm_utils.py:556-580 (stores R^T)
__global__ void rot_kernel(MpmPtrs S, float* __restrict__ Rout, const int* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const int s = perm ? perm[i] : i;
    Mat3 F, U, V;
    float sg[3];
    for (int c = 0; c < 9; ++c) F.m[c] = S.Ft[(size_t)c * S.n + i];
    svd3(F, U, sg, V);
    const Mat3 R = mat_mul_bt(U, V);
    for (int a = 0; a < 3; ++a)
        for (int b = 0; b < 3; ++b) Rout[(size_t)s * 9 + 3 * a + b] = R.m[3 * b + a];
}
// export_particle_stress_to_torch (mpm_solver_warp.py:691-692): the Kirchhoff stress of the stored,
// return-mapped F -- what the last compute_stress_from_F_trial left in particle_stress.
__global__ void stress_export_kernel(MpmPtrs S, float* __restrict__ out, const int* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const int s = perm ? perm[i] : i;
    Mat3 F;
    for (int c = 0; c < 9; ++c) F.m[c] = S.F[(size_t)c * S.n + i];
    const Mat3 tau = kirchhoff_stress(S.material[i], F, S.mu[i], S.lam[i], S.bulk[i]);
    for (int c = 0; c < 9; ++c) out[(size_t)s * 9 + c] = tau.m[c];
}
__global__ void grid_export_kernel(const float4* __restrict__ g, float* __restrict__ out, long total, int what) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const float4 q = g[i];
    if (what == 0) out[i] = q.w;
    else { out[3 * i] = q.x; out[3 * i + 1] = q.y; out[3 * i + 2] = q.z; }
}

}  // namespace pixie
