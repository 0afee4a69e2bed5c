// pixie_amd/csrc/mpm_setup_kernels.h -- MPM device code: set-up and utility kernels.
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// ------------------------------------------------------------------ set-up / utility kernels
__global__ void pmod_kernel(MpmPtrs S, StepParams sp, PModDev m) {  // overflow path (> kMaxPModFused modifiers)
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= S.n) return;
    float x[3], v[3];
    for (int d = 0; d < 3; ++d) { x[d] = S.x[d * S.n + p]; v[d] = S.v[d * S.n + p]; }
    apply_pmod(m, S.perm[p], sp.time, sp.dt, S.mass[p], x, v);
    for (int d = 0; d < 3; ++d) S.v[d * S.n + p] = v[d];
}

template <typename T>
__global__ void aos_to_soa_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int k, const int* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = perm ? perm[i] : i;
    for (int c = 0; c < k; ++c) dst[(size_t)c * n + i] = src[(size_t)s * k + c];
}
template <typename T>
__global__ void soa_to_aos_kernel(const T* __restrict__ src, T* __restrict__ dst, int n, int k, const int* perm) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = perm ? perm[i] : i;
    for (int c = 0; c < k; ++c) dst[(size_t)s * k + c] = src[(size_t)c * n + i];
}
// selection 2 = "left the grid, frozen" (our marker; the reference has no such state): cleared when the caller replaces the
// positions or re-makes the grid, so that particles that are inside again take part again
__global__ void unfreeze_kernel(int* selection, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n && selection[i] == 2) selection[i] = 0;
}
template <typename T>
__global__ void fill_kernel(T* dst, long count, T value) {
    const long i = (long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count) dst[i] = value;
}
__global__ void identity_F_kernel(float* Ft, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    for (int c = 0; c < 9; ++c) Ft[(size_t)c * n + i] = (c % 4 == 0) ? 1.0f : 0.0f;
}
// Smallest and largest positive particle mass (bit patterns of non-negative floats order like the floats).  The packed
// scatter's quantum is 2^-30 of the SUM of a work item's contribution bounds, so a node fed only by particles R times lighter
// than their neighbours in the tile is resolved to ~1e-6 R of its own mass: above a contrast of kPackMaxContrast (mpm_plan.h)
// the exact 64-bit mode is selected instead.
__global__ void mass_range_kernel(MpmPtrs S, unsigned* __restrict__ range) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    float m = (p < S.n && S.selection[p] == 0) ? S.mass[p] : 0.0f;
    unsigned lo = (m > 0.0f) ? __float_as_uint(m) : 0xffffffffu, hi = (m > 0.0f) ? __float_as_uint(m) : 0u;
    for (int off = 32; off > 0; off >>= 1) {
        lo = min(lo, (unsigned)__shfl_xor((int)lo, off, 64));
        hi = max(hi, (unsigned)__shfl_xor((int)hi, off, 64));
    }
    if ((threadIdx.x & 63) == 0) { atomicMin(range, lo); atomicMax(range + 1, hi); }
}

__global__ void mass_kernel(MpmPtrs S) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < S.n) S.mass[i] = S.density[i] * S.vol[i];
}
// compute_mu_lam_from_E_nu / compute_bulk, mpm_utils.py:282-293
__global__ void mu_lam_kernel(MpmPtrs S, int with_bulk) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const float E = S.E[i], nu = S.nu[i];
    const float mu = E / (2.0f * (1.0f + nu));
    const float lam = E * nu / ((1.0f + nu) * (1.0f - 2.0f * nu));
    S.mu[i] = mu;
    S.lam[i] = lam;
    if (with_bulk) S.bulk[i] = lam + 2.f / 3.f * mu;
}
// apply_additional_params, mpm_utils.py:591-610
__global__ void additional_params_kernel(MpmPtrs S, float3 pt, float3 sz, float E, float nu, float density, int material) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const float px = S.x[i], py = S.x[S.n + i], pz = S.x[2 * S.n + i];
    if (px > pt.x - sz.x && px < pt.x + sz.x && py > pt.y - sz.y && py < pt.y + sz.y && pz > pt.z - sz.z && pz < pt.z + sz.z) {
        S.E[i] = E; S.nu[i] = nu; S.density[i] = density; S.material[i] = material;
    }
}
// The same for a list of boxes applied in order: every particle keeps the LAST box that contains it (what N sequential
// launches of the kernel above leave behind).  Boxes are staged through LDS 256 at a time; the containment test is the
// reference's float32 expression, box by box.
__global__ __launch_bounds__(256) void additional_params_batch_kernel(MpmPtrs S, long n_boxes, const float* __restrict__ boxes,
                                                                       const float* __restrict__ params, const int* __restrict__ material) {
    __shared__ float sb[256][6];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const bool valid = i < S.n;
    const float px = valid ? S.x[i] : 0.0f, py = valid ? S.x[S.n + i] : 0.0f, pz = valid ? S.x[2 * S.n + i] : 0.0f;
    long last = -1;
    for (long b0 = 0; b0 < n_boxes; b0 += 256) {
        const long mine = b0 + threadIdx.x;
        __syncthreads();
        if (mine < n_boxes)
            for (int k = 0; k < 6; ++k) sb[threadIdx.x][k] = boxes[mine * 6 + k];
        __syncthreads();
        const int cnt = (int)min(256L, n_boxes - b0);
        if (valid)
            for (int j = 0; j < cnt; ++j) {
                const float* q = sb[j];
                if (px > q[0] - q[3] && px < q[0] + q[3] && py > q[1] - q[4] && py < q[1] + q[4] && pz > q[2] - q[5] && pz < q[2] + q[5]) last = b0 + j;
            }
    }
    if (valid && last >= 0) {
        S.E[i] = params[last * 3]; S.nu[i] = params[last * 3 + 1]; S.density[i] = params[last * 3 + 2]; S.material[i] = material[last];
    }
}
// selection kernels, mpm_utils.py:613-663
__global__ void select_kernel(MpmPtrs S, PModDev m, float3 size, float half_height, float radius, int* mask) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= S.n) return;
    const float o[3] = {S.x[i] - m.point[0], S.x[S.n + i] - m.point[1], S.x[2 * S.n + i] - m.point[2]};
    int sel;
    if (m.type == PIXIE_PM_ROTATION) {
        const float dn = o[0] * m.normal[0] + o[1] * m.normal[1] + o[2] * m.normal[2];
        const float hx = o[0] - dn * m.normal[0], hy = o[1] - dn * m.normal[1], hz = o[2] - dn * m.normal[2];
        sel = (fabsf(dn) < half_height && sqrtf(hx * hx + hy * hy + hz * hz) < radius) ? 1 : 0;
    } else {
        sel = (fabsf(o[0]) < size.x && fabsf(o[1]) < size.y && fabsf(o[2]) < size.z) ? 1 : 0;
    }
    mask[S.perm[i]] = sel;  // masks are kept in the caller's order
}
// compute_cov_from_F, mpm_utils.py:529-553

}  // namespace pixie
