// pixie_amd/csrc/density_field_math.h -- the arithmetic of the proposal density field (density_field.hip) after the hash grid: the
// 16-wide layers, trunc_exp and its derivative rule, and the host policy (launch geometry, slab count, byte sizes), as
// __host__ __device__ functions, so that tests/host_harness/density_field_math_host.cpp runs the same lines on the CPU (g++
// -ffp-contract=off) against the NumPy restatement of tests/_density_field_ref.py.  The front end (affine, contraction or aabb,
// selector, cells, corners) is hashgrid_math.h, unchanged.
//
//   layer     z_j = fmaf(W[j][K-1], x_(K-1), ... fmaf(W[j][0], x_0, b_j or 0)): one chain per unit, k in index order.  The kernel
//             feeds the first layer column by column as each level's features arrive (layer_column), which is the same chain.
//   hidden    ReLU; the width is exactly 16; 0, 1 or 2 hidden layers (0: the reference's use_linear), then one output h
//   density   average_init_density * exp(h) * selector; a point whose selector is 0 gets exactly 0 and is never evaluated
//   backward  trunc_exp's rule: dL/dh = (g * average_init_density) * exp(clamp(h, -15, 15)), not the saved output; 0 when the
//             selector is 0
//   policy    the backward's workgroups walk the points in tiles of 256 with a stride of the grid; a workgroup is one SLAB of the
//             weight and bias gradients: one partial per slab, summed in slab order.  slab_count is a pure function of n.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define DF_HD __host__ __device__ inline
#else
#define DF_HD inline
#endif

namespace pixie {
namespace df {

constexpr int kWidth = 16;                       // hidden units
constexpr int kMaxHidden = 2;
constexpr int kMaxInput = 64;                    // levels * features_per_level
constexpr int kThreads = 256;                    // a workgroup, and a tile of points: a lane per point
constexpr int kMaxForwardBlocks = 2048;          // 8 workgroups per CU on 256 CUs
constexpr int kMaxSlabs = 1024;                  // the backward's workgroups: 4 per CU on 256 CUs, more than its LDS lets reside at once
                                                 // (58 KB each for the reference shape: 2 per CU), so a CU that finishes early takes another
constexpr int64_t kMaxPoints = (int64_t)1 << 24; // hashgrid_grad_math.h's limit
constexpr int kHeaderBytes = 256;

// ---- layers ---------------------------------------------------------------------------------------------------------------
DF_HD void layer_seed(const float* bias, float* acc) {                       // bias: kWidth floats or null
    for (int j = 0; j < kWidth; ++j) acc[j] = bias != nullptr ? bias[j] : 0.0f;
}

// input column k of a 16-wide layer: wk[j] = W[j][k]
DF_HD void layer_column(const float* wk, float x, float* acc) {
    for (int j = 0; j < kWidth; ++j) acc[j] = fmaf(wk[j], x, acc[j]);
}

DF_HD float relu(float z) { return z > 0.0f ? z : 0.0f; }

// z[j] = chain over k of W[j][k] x[k] from b[j]; W (kWidth, K) row-major
DF_HD void layer(const float* W, const float* bias, int K, const float* x, float* z) {
    for (int j = 0; j < kWidth; ++j) {
        float a = bias != nullptr ? bias[j] : 0.0f;
        for (int k = 0; k < K; ++k) a = fmaf(W[j * K + k], x[k], a);
        z[j] = a;
    }
}

// h = chain over k of w[k] x[k] from b
DF_HD float output_unit(const float* w, const float* bias, int K, const float* x) {
    float a = bias != nullptr ? bias[0] : 0.0f;
    for (int k = 0; k < K; ++k) a = fmaf(w[k], x[k], a);
    return a;
}

// The network after the encoding: x (in_dim) -> h.  weight[i] / bias[i] as the descriptor holds them; zs (n_hidden * kWidth) receives
// the hidden pre-activations when not null.
DF_HD float network(int n_hidden, int in_dim, const float* const* weight, const float* const* bias, const float* x, float* zs) {
    float a[kWidth], b[kWidth];
    const float* src = x;
    int K = in_dim;
    for (int i = 0; i < n_hidden; ++i) {
        float* dst = (i & 1) ? b : a;
        layer(weight[i], bias[i], K, src, dst);
        for (int j = 0; j < kWidth; ++j) {
            if (zs != nullptr) zs[i * kWidth + j] = dst[j];
            dst[j] = relu(dst[j]);
        }
        src = dst;
        K = kWidth;
    }
    return output_unit(weight[n_hidden], bias[n_hidden], K, src);
}

// ---- trunc_exp ------------------------------------------------------------------------------------------------------------
DF_HD float density_of(float h, float average_init_density) { return average_init_density * expf(h); }

DF_HD float clamp15(float h) { return fminf(fmaxf(h, -15.0f), 15.0f); }

// dL/dh from g = dL/d density
DF_HD float dh_of(float g, float h, float average_init_density, int selector) {
    return selector ? (g * average_init_density) * expf(clamp15(h)) : 0.0f;
}

// ---- host policy ----------------------------------------------------------------------------------------------------------
DF_HD int64_t tiles_of(int64_t n) { return (n + kThreads - 1) / kThreads; }

DF_HD int forward_blocks(int64_t n) {
    const int64_t t = tiles_of(n);
    return (int)(t < 1 ? 1 : (t > kMaxForwardBlocks ? kMaxForwardBlocks : t));
}

// slabs of the weight and bias gradients = workgroups of the backward; slab b owns tiles b, b + slabs, b + 2 slabs, ...
DF_HD int slab_count(int64_t n) {
    const int64_t t = tiles_of(n);
    return (int)(t < 1 ? 1 : (t > kMaxSlabs ? kMaxSlabs : t));
}

// floats of one slab's partial: every weight and bias of the network, biases included whether or not the network has them
//   n_hidden >= 1: W0 (16, in_dim) | b0 (16) | [W1 (16, 16) | b1 (16)] | w_out (16) | b_out (1)
//   n_hidden == 0: w_out (in_dim) | b_out (1)
DF_HD int param_count(int in_dim, int n_hidden) {
    if (n_hidden == 0) return in_dim + 1;
    return kWidth * in_dim + kWidth + (n_hidden - 1) * (kWidth * kWidth + kWidth) + kWidth + 1;
}

// offset of layer i's weights inside a partial; its bias follows its weights
DF_HD int weight_offset(int in_dim, int n_hidden, int i) {
    if (i == 0) return 0;
    int at = kWidth * in_dim + kWidth;
    if (i == 2) at += kWidth * kWidth + kWidth;
    return at;
}

DF_HD int layer_out(int n_hidden, int i) { return i == n_hidden ? 1 : kWidth; }
DF_HD int layer_in(int in_dim, int i) { return i == 0 ? in_dim : kWidth; }

DF_HD int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }

// The forward is recomputed from the positions in the backward: nothing is saved per point.
DF_HD int64_t saved_bytes(int64_t /*n*/) { return 0; }

// scratch of the backward: header | masked unit positions [3][n] | dX of the grid columns [in_dim][n] | slab partials | accumulators
struct Scratch {
    int64_t pos, dxg, part, acc, total;
};

DF_HD Scratch scratch_layout(int64_t n, int in_dim, int n_hidden, int64_t table_rows, int features_per_level) {
    Scratch L;
    L.pos = kHeaderBytes;
    L.dxg = L.pos + round256(4 * 3 * n);
    L.part = L.dxg + round256(4 * (int64_t)in_dim * n);
    L.acc = L.part + round256(4 * (int64_t)slab_count(n) * param_count(in_dim, n_hidden));
    L.total = L.acc + round256(8 * table_rows * features_per_level);
    return L;
}

}  // namespace df
}  // namespace pixie
