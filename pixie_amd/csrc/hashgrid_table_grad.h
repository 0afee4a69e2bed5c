// pixie_amd/csrc/hashgrid_table_grad.h -- the device side of the hash table's fixed-point gradient (hashgrid_grad_math.h), shared by the
// 64-wide networks (field_query_backward.hip) and the proposal density field (density_field.hip): the scatter of one (point, level,
// corner, feature) item and the finalise kernel.  Everything sits in an anonymous namespace: every function is internal to
// the file that includes it.
//
//   scatter   one lane per (point, level, corner, feature): consecutive lanes are the F features of one row, consecutive groups the 8
//             corners of one cell.  c = w_corner dX[column] in float32, llrint(c 2^s) added by a no-return 64-bit integer atomic; the
//             shift s comes from the device-side maximum in the scratch header.  Desc is a descriptor with n_levels,
//             features_per_level and level[]; fetch(point, pp) gives the unit-cube position the forward's cell was taken at.
//   finalise  d_table[i] = float32(double(acc[i]) 2^-s), NaN everywhere if the maximum was not finite; the header receives s and the state
#pragma once
#include <hip/hip_runtime.h>

#include <cstdint>

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
    hg::Level lv;
    lv.scale = m.level[l].scale; lv.shift = m.level[l].shift; lv.res = m.level[l].res;
    lv.size = m.level[l].size; lv.offset = m.level[l].offset; lv.dense = m.level[l].dense;
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

}  // namespace
