// pixie_amd/csrc/mpm_dense_grid_kernels.h -- MPM device code: grid export while a P2G is pending, and the dense grid kernel.
// Part of the mpm.hip translation unit (included there, in a fixed order: the kernels' definition order is the order of the code object).
#pragma once

namespace pixie {

// export of grid_m / grid_v_in while a P2G is pending (tiles not yet consumed by the grid kernel)
__global__ __launch_bounds__(64) void grid_export_pending_kernel(MpmPtrs S, float* __restrict__ out, int what) {
    const int Bz = blockIdx.x % S.nbk, By = (blockIdx.x / S.nbk) % S.nbk, Bx = blockIdx.x / (S.nbk * S.nbk);
    const int lx = threadIdx.x >> 4, ly = (threadIdx.x >> 2) & 3, lz = threadIdx.x & 3;
    const int ix = Bx * kBS + lx, iy = By * kBS + ly, iz = Bz * kBS + lz;
    const bool inside = ix < S.ng && iy < S.ng && iz < S.ng;
    const size_t idx = ((size_t)ix * S.ng + iy) * S.ng + iz;
    float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
    if (inside) g = S.gin[idx];
    g = gather_node<4>(S, neighbour_items(S, Bx, By, Bz), lx, ly, lz, g);
    if (!inside) return;
    if (what == 0) out[idx] = g.w;
    else { out[3 * idx] = g.x; out[3 * idx + 1] = g.y; out[3 * idx + 2] = g.z; }
}

__global__ __launch_bounds__(256) void mpm_grid_kernel(MpmPtrs S, StepParams sp, BCSet bcs, int normalise) {
    const long total = (long)S.ng * S.ng * S.ng;
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int iz = (int)(idx % S.ng);
    const int iy = (int)((idx / S.ng) % S.ng);
    const int ix = (int)(idx / ((long)S.ng * S.ng));
    float v[3] = {0.0f, 0.0f, 0.0f};
    if (normalise) {
        const float4 g = S.gin[idx];
        if (g.w > 1e-15f) {
            const float inv = 1.0f / g.w;
            v[0] = g.x * inv + sp.dt * sp.g[0];
            v[1] = g.y * inv + sp.dt * sp.g[1];
            v[2] = g.z * inv + sp.dt * sp.g[2];
        }
        if (sp.do_damping) { v[0] *= sp.damping; v[1] *= sp.damping; v[2] *= sp.damping; }
        if (g.x != 0.0f || g.y != 0.0f || g.z != 0.0f || g.w != 0.0f) S.gin[idx] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    } else {
        const float4 o = S.gout[idx];
        v[0] = o.x; v[1] = o.y; v[2] = o.z;
    }
    for (int k = 0; k < bcs.n; ++k) apply_bc(bcs.bc[k], ix, iy, iz, S.ng, S.dx, sp.time, sp.dt, v);
    S.gout[idx] = make_float4(v[0], v[1], v[2], 0.0f);
}

}  // namespace pixie
