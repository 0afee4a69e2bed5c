// pixie_amd/csrc/field_query_body.h -- the device body of one "hash-grid encoding -> 64-wide MLP" tile, shared by the query
// (field_query.hip) and the training pass (field_query_backward.hip): encode tile, LDS layers on v_mfma_f32_32x32x2_f32, streamed
// output layer, and the descriptor check both boundaries apply.  Included inside an anonymous namespace's translation unit; every
// function is internal to the file that includes it.  The tiling and the LDS layout are described at the top of field_query.hip.
#pragma once
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "hashgrid_check.h"
#include "hashgrid_math.h"
#include "hashmlp_plan.h"

namespace {

using namespace pixie;
typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int P = 64;                            // points per workgroup
constexpr int THREADS = 256;
constexpr int KMAX = PIXIE_HASHMLP_MAX_INPUT;    // rows of the input buffer
constexpr int WLD = 65;                          // row pitch of the staged weight chunk [k][out]
constexpr int OLD = 68;                          // row pitch of the transposed output tile [point][out]
// LDS, in floats: X | H | WL | pos[3][P] | aux[P]
constexpr int X_OFF = 0, H_OFF = KMAX * P, WL_OFF = H_OFF + 64 * P, POS_OFF = WL_OFF + 64 * WLD, AUX_OFF = POS_OFF + 3 * P;
constexpr int LDS_FLOATS = AUX_OFF + P;
constexpr size_t LDS_BYTES = LDS_FLOATS * sizeof(float);     // 75008: two workgroups per CU
static_assert(P * OLD <= KMAX * P, "the output tile reuses the input buffer");

static_assert(P == hmp::kTile, "hashmlp_plan.h plans for this tile");

// pos[3][P] = the tile's positions as given (past the end, or without positions: 0), complete on return
__device__ inline void load_tile_positions(const float* d_positions, int64_t tile0, int64_t n, float* pos) {
    const int tid = threadIdx.x;
    if (tid < 3 * P) {
        const int p = tid / 3, a = tid - 3 * p;
        pos[a * P + p] = (d_positions != nullptr && tile0 + p < n) ? d_positions[(tile0 + p) * 3 + a] : 0.f;
    }
    __syncthreads();
}

// X[column][point] of the tile's rows.  pos: LDS [3][P] unit-cube positions.
__device__ void encode_tile(const pixie_hashmlp_desc& m, const float* pos, const float* d_extra, int64_t tile0, int64_t n, float* X) {
    const int tid = threadIdx.x, F = m.features_per_level;
    for (int item = tid; item < m.n_levels * P; item += THREADS) {
        const int l = item >> 6, p = item & (P - 1);
        const hg::Level lv = hg::level_of(m.level[l]);
        const float pp[3] = {pos[p], pos[P + p], pos[2 * P + p]};
        const hg::Cell s = hg::cell_of(lv, pp);
        float f[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wk = hg::corner_weight(s, k);
            const float* row = m.d_table + (size_t)hg::corner_row_k(lv, s, k) * F;
            if (F == 2) {
                const float2 v = *reinterpret_cast<const float2*>(row);
                f[0] += wk * v.x; f[1] += wk * v.y;
            } else {
                const float4 v = *reinterpret_cast<const float4*>(row);
                f[0] += wk * v.x; f[1] += wk * v.y; f[2] += wk * v.z; f[3] += wk * v.w;
                if (F == 8) {
                    const float4 u = *reinterpret_cast<const float4*>(row + 4);
                    f[4] += wk * u.x; f[5] += wk * u.y; f[6] += wk * u.z; f[7] += wk * u.w;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i)
            if (i < F) X[(l * F + i) * P + p] = f[i];
    }
    int base = m.n_levels * F;
    for (int item = tid; item < 6 * m.n_frequencies * P; item += THREADS) {
        const int j = item >> 6, p = item & (P - 1);
        const float pp[3] = {pos[p], pos[P + p], pos[2 * P + p]};
        const float a = hg::frequency_arg(pp, j, m.n_frequencies);
        X[(base + j) * P + p] = (j & 1) ? cosf(a) : sinf(a);
    }
    base += 6 * m.n_frequencies;
    for (int item = tid; item < m.n_extra * P; item += THREADS) {
        const int p = item / m.n_extra, e = item - p * m.n_extra;
        X[(base + e) * P + p] = tile0 + p < n ? d_extra[(tile0 + p) * m.n_extra + e] : 0.f;
    }
    base += m.n_extra;
    if (base & 1)                                 // the K loop runs in pairs: the odd row meets zero weights and must be finite
        for (int p = tid; p < P; p += THREADS) X[base * P + p] = 0.f;
}

// The 64 x 64 weight chunk wl[k][o] = W[o0 + o][k0 + k] (zero outside the matrix) in two steps, so that a thread's 16 loads are in
// flight together, and, in the output layer, during the previous chunk's matrix instructions: registers first, LDS second.
constexpr int WPT = 64 * 64 / THREADS;           // weights per thread

__device__ inline void load_weights(const float* W, int out_dim, int in_dim, int o0, int k0, float (&v)[WPT]) {
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
        const int i = threadIdx.x + j * THREADS, k = i & 63, o = i >> 6;
        v[j] = (o0 + o < out_dim && k0 + k < in_dim) ? W[(size_t)(o0 + o) * in_dim + k0 + k] : 0.f;
    }
}

__device__ inline void store_weights(const float (&v)[WPT], float* wl) {
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
        const int i = threadIdx.x + j * THREADS, k = i & 63, o = i >> 6;
        wl[k * WLD + o] = v[j];
    }
}

// C/D layout of v_mfma_f32_32x32x2_f32: lane (r = lane & 31, hi = lane >> 5), register g holds row (g & 3) + 8 (g >> 2) + 4 hi, column r
__device__ inline int acc_row(int g, int hi) { return (g & 3) + 8 * (g >> 2) + 4 * hi; }

__device__ inline f32x16 bias_seed(const float* bias, int out_dim, int row0, int hi) {
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int o = row0 + acc_row(g, hi);
        acc[g] = (bias != nullptr && o < out_dim) ? bias[o] : 0.f;
    }
    return acc;
}

// dst[o][point] = act(W[o][:] . src[:][point] + bias[o]) for o < 64 (rows >= out_dim come out as zeros); src, dst: LDS [rows][P], distinct
__device__ void lds_layer(const float* W, const float* bias, int out_dim, int in_dim, bool relu, const float* src, float* dst, float* wl) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63, r = lane & 31, hi = lane >> 5, mb = wave & 1, nb = wave >> 1;
    f32x16 acc = bias_seed(bias, out_dim, mb * 32, hi);
    float wv[WPT];
    for (int k0 = 0; k0 < in_dim; k0 += 64) {
        load_weights(W, out_dim, in_dim, 0, k0, wv);
        __syncthreads();                          // src is complete; the previous chunk of wl has been read
        store_weights(wv, wl);
        __syncthreads();
        const int kl = in_dim - k0 < 64 ? in_dim - k0 : 64, pairs = (kl + 1) >> 1;
        for (int kp = 0; kp < pairs; ++kp) {
            const float a = wl[(2 * kp + hi) * WLD + mb * 32 + r];
            const float b = src[(k0 + 2 * kp + hi) * P + nb * 32 + r];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const float v = acc[g];
        dst[(mb * 32 + acc_row(g, hi)) * P + nb * 32 + r] = relu ? fmaxf(v, 0.f) : v;
    }
}

// Runs the hidden layers from `src` (in_dim rows) and returns the buffer that holds the last hidden activations.
__device__ const float* hidden_layers(const pixie_hashmlp_desc& m, int in_dim, const float* src, float* X, float* H, float* wl) {
    for (int i = 0; i < m.n_hidden; ++i) {
        float* dst = (src >= H && src < H + 64 * P) ? X : H;
        lds_layer(m.d_weight[i], m.d_bias[i], 64, i == 0 ? in_dim : 64, true, src, dst, wl);
        src = dst;
    }
    return src;
}

__device__ inline float out_act(float v, int act) {
    if (act == 1) return 1.f / (1.f + expf(-v));
    if (act == 2) return expf(v);
    return v;
}

// The output layer from the 64 hidden rows of `src`.  ot: LDS [P][OLD], may overlap src (src is in registers before ot is written).
// HALF: d_out is float16 (n, out_dim) and every value is multiplied by scale[point] (LDS) first; otherwise float32.
template <bool HALF>
__device__ void output_layer(const pixie_hashmlp_desc& m, const float* src, float* ot, float* wl, const float* scale, void* d_out,
                             int64_t tile0, int64_t n) {
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hi = lane >> 5, mb = wave & 1, nb = wave >> 1;
    const float* W = m.d_weight[m.n_hidden];
    const float* bias = m.d_bias[m.n_hidden];
    const int out_dim = m.out_dim, act = m.out_activation;
    float b[32];
    __syncthreads();                              // the last hidden layer's rows come from both waves of a column half
#pragma unroll
    for (int kp = 0; kp < 32; ++kp) b[kp] = src[(2 * kp + hi) * P + nb * 32 + r];
    const int p = tid >> 2, cs = (tid & 3) * 16;   // the store phase: 4 threads per point, 16 channels each
    const int64_t gp = tile0 + p;
    const bool vec = HALF ? (out_dim % 8 == 0) : (out_dim % 4 == 0);
    float wv[WPT];
    load_weights(W, out_dim, 64, 0, 0, wv);
    for (int o0 = 0; o0 < out_dim; o0 += 64) {
        __syncthreads();                          // b is loaded; the previous tile has been stored; wl is free
        store_weights(wv, wl);
        __syncthreads();
        if (o0 + 64 < out_dim) load_weights(W, out_dim, 64, o0 + 64, 0, wv);      // the next chunk, under this chunk's matrix work
        f32x16 acc = bias_seed(bias, out_dim, o0 + mb * 32, hi);
#pragma unroll
        for (int kp = 0; kp < 32; ++kp) {
            const float a = wl[(2 * kp + hi) * WLD + mb * 32 + r];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b[kp], acc, 0, 0, 0);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g)
            *reinterpret_cast<float4*>(&ot[(nb * 32 + r) * OLD + mb * 32 + 8 * g + 4 * hi]) =
                make_float4(acc[4 * g], acc[4 * g + 1], acc[4 * g + 2], acc[4 * g + 3]);
        __syncthreads();
        if (gp < n) {
            const float s = HALF ? scale[p] : 1.f;
            float v[16];
#pragma unroll
            for (int c = 0; c < 16; c += 4) {
                const float4 t = *reinterpret_cast<const float4*>(&ot[p * OLD + cs + c]);
                v[c] = t.x; v[c + 1] = t.y; v[c + 2] = t.z; v[c + 3] = t.w;
            }
#pragma unroll
            for (int c = 0; c < 16; ++c) {
                v[c] = out_act(v[c], act);
                if (HALF) v[c] = v[c] * s;
            }
            const int o = o0 + cs;
            if (HALF) {
                __half* out = reinterpret_cast<__half*>(d_out) + gp * out_dim;
                if (vec) {
#pragma unroll
                    for (int c = 0; c < 16; c += 8) {
                        if (o + c < out_dim) {
                            union { __half h[8]; uint4 u; } pk;
#pragma unroll
                            for (int e = 0; e < 8; ++e) pk.h[e] = __float2half_rn(v[c + e]);
                            *reinterpret_cast<uint4*>(out + o + c) = pk.u;
                        }
                    }
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (o + c < out_dim) out[o + c] = __float2half_rn(v[c]);
                }
            } else {
                float* out = reinterpret_cast<float*>(d_out) + gp * out_dim;
                if (vec) {
#pragma unroll
                    for (int c = 0; c < 16; c += 4)
                        if (o + c < out_dim) *reinterpret_cast<float4*>(out + o + c) = make_float4(v[c], v[c + 1], v[c + 2], v[c + 3]);
                } else {
#pragma unroll
                    for (int c = 0; c < 16; ++c)
                        if (o + c < out_dim) out[o + c] = v[c];
                }
            }
        }
    }
}

int check_desc(const pixie_hashmlp_desc* m, const char* what) {
    PX_REQUIRE(m != nullptr, "%s: null descriptor", what);
    PX_REQUIRE(m->n_levels >= 0 && m->n_levels <= PIXIE_HASHMLP_MAX_LEVELS, "%s: n_levels %d outside 0..%d", what, m->n_levels, PIXIE_HASHMLP_MAX_LEVELS);
    if (m->n_levels > 0) {
        PX_REQUIRE(m->features_per_level == 2 || m->features_per_level == 4 || m->features_per_level == 8,
                   "%s: features_per_level %d is not 2, 4 or 8", what, m->features_per_level);
        if (check_grid_table(*m, what)) return 1;
    }
    PX_REQUIRE(m->n_frequencies >= 0 && m->n_frequencies <= 8, "%s: n_frequencies %d outside 0..8", what, m->n_frequencies);
    PX_REQUIRE(m->n_extra >= 0 && m->n_extra <= PIXIE_HASHMLP_MAX_INPUT, "%s: n_extra %d outside 0..%d", what, m->n_extra, PIXIE_HASHMLP_MAX_INPUT);
    const int width = hg::input_width(*m);
    PX_REQUIRE(width >= 1 && width <= PIXIE_HASHMLP_MAX_INPUT, "%s: input row of %d columns outside 1..%d", what, width, PIXIE_HASHMLP_MAX_INPUT);
    PX_REQUIRE(m->n_hidden >= 1 && m->n_hidden <= PIXIE_HASHMLP_MAX_LAYERS - 1, "%s: %d hidden layers outside 1..%d (each 64 wide)", what, m->n_hidden,
               PIXIE_HASHMLP_MAX_LAYERS - 1);
    PX_REQUIRE(m->out_dim >= 1 && m->out_dim <= PIXIE_HASHMLP_MAX_OUTPUT, "%s: out_dim %d outside 1..%d", what, m->out_dim, PIXIE_HASHMLP_MAX_OUTPUT);
    PX_REQUIRE(m->out_activation >= 0 && m->out_activation <= 2, "%s: out_activation %d is not 0 (none), 1 (sigmoid) or 2 (exp)", what, m->out_activation);
    for (int i = 0; i <= m->n_hidden; ++i) PX_REQUIRE(m->d_weight[i] != nullptr, "%s: d_weight[%d] is null", what, i);
    return 0;
}

template <class K>
int prepare(K kern) {
    PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(kern)));
    return 0;
}

}  // namespace
