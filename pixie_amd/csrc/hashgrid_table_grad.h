// pixie_amd/csrc/hashgrid_table_grad.h -- the training back end shared by the 64-wide networks (field_query_backward.hip) and the
// proposal density field (density_field.hip): the device side of the hash table's fixed-point gradient (hashgrid_grad_math.h) and the
// two host steps both backward entry points share.  Everything sits in an anonymous namespace: every function is internal to the file
// that includes it.
//
//   scatter   one lane per (point, level, corner, feature): consecutive lanes are the F features of one row, consecutive groups the 8
//             corners of one cell.  c = w_corner dX[column] in float32, llrint(c 2^s) added by a no-return 64-bit integer atomic; the
//             shift s comes from the device-side maximum in the scratch header.  Desc is a descriptor with n_levels,
//             features_per_level and level[]; fetch(point, pp) gives the unit-cube position the forward's cell was taken at.
//   finalise  d_table[i] = float32(double(acc[i]) 2^-s), NaN everywhere if the maximum was not finite; the header receives s and the state
//   host      zero_empty_grads is the n == 0 branch of a grads struct (d_table, d_weight[], d_bias[]); finish_table_grad launches the
//             file's own scatter kernel and the finalise.  Before it each file checks, carves and zeroes its scratch and launches its
//             own kernels.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>
#include <utility>

#include "common.h"
#include "hashgrid_grad_math.h"
#include "hashgrid_math.h"

namespace {

template <class Desc, class Fetch>
__device__ inline void table_scatter_item(const Desc& m, Fetch fetch, int64_t n, const float* d_dxg, const unsigned int* d_header,
                                          unsigned long long* d_acc, int threads) {
    using namespace pixie;
    const unsigned int bits = d_header[0];
    if (hgg::state_of(bits) != hgg::kNormal) return;
    const int s = hgg::shift_of(bits, n);
    const int F = m.features_per_level, per = 8 * F;
    const int64_t t = (int64_t)blockIdx.x * threads + threadIdx.x;
    if (t >= n * m.n_levels * per) return;
    const int f = (int)(t % F), k = (int)((t / F) % 8);
    const int64_t pl = t / per, point = pl % n;
    const int l = (int)(pl / n);
    const hg::Level lv = hg::level_of(m.level[l]);
    float pp[3];
    fetch(point, pp);
    const hg::Cell cell = hg::cell_of(lv, pp);
    const float c = hg::corner_weight(cell, k) * d_dxg[(int64_t)(l * F + f) * n + point];
    const long long q = hgg::quantise(c, s);
    if (q != 0) atomicAdd(d_acc + (size_t)hg::corner_row_k(lv, cell, k) * F + f, (unsigned long long)q);
}

__global__ void table_finalise_kernel(const long long* d_acc, int64_t count, int64_t n, unsigned int* d_header, float* d_table) {
    using namespace pixie;
    const unsigned int bits = d_header[0];
    const int state = hgg::state_of(bits), s = state == hgg::kNormal ? hgg::shift_of(bits, n) : 0;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i == 0) {
        reinterpret_cast<int*>(d_header)[1] = s;
        reinterpret_cast<int*>(d_header)[2] = state;
    }
    if (i < count) d_table[i] = state == hgg::kNonFinite ? __int_as_float(0x7fc00000) : hgg::finalise(d_acc[i], s);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
// the empty sum (n == 0): every gradient asked for is zero.  shape(i) gives layer i's (out, in).
template <class Grads, class Shape>
int zero_empty_grads(const Grads& g, int n_layers, size_t table_floats, Shape shape, hipStream_t st) {
    if (g.d_table != nullptr) PX_CHECK_HIP(hipMemsetAsync(g.d_table, 0, 4 * table_floats, st));
    for (int i = 0; i < n_layers; ++i) {
        const std::pair<int, int> oi = shape(i);
        if (g.d_weight[i] != nullptr) PX_CHECK_HIP(hipMemsetAsync(g.d_weight[i], 0, 4 * (size_t)oi.first * oi.second, st));
        if (g.d_bias[i] != nullptr) PX_CHECK_HIP(hipMemsetAsync(g.d_bias[i], 0, 4 * (size_t)oi.first, st));
    }
    return 0;
}

// scatter: the file's kernel around table_scatter_item, (m, d_pos, n, d_dxg, header, acc), launched with `threads` per workgroup
template <class Kernel, class Desc>
int finish_table_grad(Kernel scatter, int threads, const Desc& m, const float* d_pos, int64_t n, const float* d_dxg, unsigned int* header,
                      unsigned long long* acc, float* d_table, hipStream_t st) {
    const int64_t items = n * m.n_levels * 8 * m.features_per_level, count = m.table_rows * m.features_per_level;
    hipLaunchKernelGGL(scatter, dim3((unsigned)((items + threads - 1) / threads)), dim3(threads), 0, st, m, d_pos, n, d_dxg, (const unsigned int*)header, acc);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(table_finalise_kernel, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, st, (const long long*)acc, count, n, header, d_table);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

}  // namespace
