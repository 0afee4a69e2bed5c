// pixie_amd/csrc/field_query.hip -- NeRF feature-field query: multiresolution hash grid -> 64-wide MLP, fused.
//
// Replaces the reference's tiny-cuda-nn evaluation of the three F3RM networks behind pixie/voxel/voxelize.py:
// extract_clip_voxel_grid (:17-141), which queries f3rm_robot/field_adapter.py (:28-72) 4096 points at a time with four network
// passes, three device-to-host copies and an empty_cache() per batch.
//
// One workgroup (4 waves) owns a tile of P = 64 points from the position to the stored output:
//   encode   one (level, point) item per thread: hashgrid_math.h's cell, 8 corner rows (vector loads of F floats), trilinear sum;
//            then the frequency columns and the extra input columns.  The row lands in LDS as X[column][point].
//   hidden   out[64][64 points] = W[64][K] X[K][64]: each wave one 32 x 32 block on v_mfma_f32_32x32x2_f32 (exact float32
//            products, float32 accumulate), the accumulator seeded with the bias.  W comes through LDS in 64-column chunks, transposed
//            on the way (row pitch 65: the transposing writes and the unit-stride reads are both conflict-free).  Activations
//            ping-pong between two LDS buffers in the same [channel][point] layout, which is the B-operand layout.
//   output   the wave's B operand (64 hidden channels of its 32 points) sits in 32 registers for the whole layer; the (out, 64)
//            weights stream through the same LDS chunk 64 output columns at a time; each 64 x 64 result tile is transposed
//            through LDS so that a point's channels leave as 16-byte stores.
// Nothing wider than the outputs reaches HBM: no (N, K) row, no (N, 64) hidden, no (N, C) float32 grid.
//
// pixie_field_voxelize is two launches of that tile body: (1) lattice position -> selector -> density net, whose output tile stays
// in LDS, -> density, alpha (float16 + the float32 scratch) -> colour head on the geometry columns -> rgb; (2) lattice position ->
// feature net -> x alpha -> float16.  Built with -ffp-contract=off: the positions and cells round as hashgrid_math.h does on the host.
#include <hip/hip_fp16.h>
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "hashgrid_math.h"

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

__device__ inline int input_width(const pixie_hashmlp_desc& m) {
    return m.n_levels * m.features_per_level + 6 * m.n_frequencies + m.n_extra;
}

// X[column][point] of the tile's rows.  pos: LDS [3][P] unit-cube positions.
__device__ void encode_tile(const pixie_hashmlp_desc& m, const float* pos, const float* d_extra, int64_t tile0, int64_t n, float* X) {
    const int tid = threadIdx.x, F = m.features_per_level;
    for (int item = tid; item < m.n_levels * P; item += THREADS) {
        const int l = item >> 6, p = item & (P - 1);
        hg::Level lv;
        lv.scale = m.level[l].scale; lv.shift = m.level[l].shift; lv.res = m.level[l].res;
        lv.size = m.level[l].size; lv.offset = m.level[l].offset; lv.dense = m.level[l].dense;
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

__global__ __launch_bounds__(THREADS) void hashmlp_forward_kernel(const pixie_hashmlp_desc m, const float* d_positions, const float* d_extra,
                                                                  int64_t n, float* d_out) {
    extern __shared__ float lds[];
    float *X = lds + X_OFF, *H = lds + H_OFF, *wl = lds + WL_OFF, *pos = lds + POS_OFF;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    const int tid = threadIdx.x;
    if (tid < 3 * P) {
        const int p = tid / 3, a = tid - 3 * p;
        pos[a * P + p] = (d_positions != nullptr && tile0 + p < n) ? d_positions[(tile0 + p) * 3 + a] : 0.f;
    }
    __syncthreads();
    encode_tile(m, pos, d_extra, tile0, n, X);
    const float* hid = hidden_layers(m, input_width(m), X, X, H, wl);
    output_layer<false>(m, hid, X, wl, nullptr, d_out, tile0, n);
}

// pos[3][P] = the unit-cube position of the tile's points (past the end: 0), multiplied by the selector if `masked`; aux[P] = the
// selector.  The world position is row g of d_points if given, else voxel g of the lattice.
__device__ void tile_positions(const pixie_field_voxelize_desc& v, const float* d_points, int64_t tile0, int64_t n, bool masked, float* pos,
                               float* aux) {
    const int p = threadIdx.x;
    if (p < P) {
        float q[3] = {0.f, 0.f, 0.f};
        int sel = 0;
        const int64_t g = tile0 + p;
        if (g < n) {
            float x[3];
            if (d_points != nullptr) {
                x[0] = d_points[3 * g]; x[1] = d_points[3 * g + 1]; x[2] = d_points[3 * g + 2];
            } else {
                const int k = (int)(g % v.w), j = (int)((g / v.w) % v.h), i = (int)(g / ((int64_t)v.w * v.h));
                x[0] = v.d_axis_x != nullptr ? v.d_axis_x[i] : hg::lattice_coord(v.min_bounds[0], v.voxel_size, i);
                x[1] = v.d_axis_y != nullptr ? v.d_axis_y[j] : hg::lattice_coord(v.min_bounds[1], v.voxel_size, j);
                x[2] = v.d_axis_z != nullptr ? v.d_axis_z[k] : hg::lattice_coord(v.min_bounds[2], v.voxel_size, k);
            }
            hg::affine(v.world_to_nerf, x, q);
            if (v.contraction) hg::contract_linf(q); else hg::normalise_aabb(v.aabb, q);
            sel = hg::selector(q);
        }
        const float f = masked ? (float)sel : 1.f;
        pos[p] = q[0] * f; pos[P + p] = q[1] * f; pos[2 * P + p] = q[2] * f;
        aux[p] = (float)sel;
    }
}

// HALF: the lattice call's float16 outputs; otherwise the point query's float32 ones.  Null outputs are skipped; without d_rgb the
// colour head does not run.
template <bool HALF>
__global__ __launch_bounds__(THREADS) void field_density_color_kernel(const pixie_field_voxelize_desc v, const float* d_points, int64_t n, float delta,
                                                                      void* d_alpha, void* d_rgb, float* d_density, float* d_scratch) {
    extern __shared__ float lds[];
    float *X = lds + X_OFF, *H = lds + H_OFF, *wl = lds + WL_OFF, *pos = lds + POS_OFF, *aux = lds + AUX_OFF;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    tile_positions(v, d_points, tile0, n, true, pos, aux);
    __syncthreads();
    encode_tile(v.density, pos, nullptr, tile0, n, X);
    const float* hid = hidden_layers(v.density, input_width(v.density), X, X, H, wl);
    float* geo = (hid >= H && hid < H + 64 * P) ? X : H;         // [h_0 | geometry columns | zero rows][P]
    const int last = v.density.n_hidden;
    lds_layer(v.density.d_weight[last], v.density.d_bias[last], v.density.out_dim, 64, false, hid, geo, wl);
    __syncthreads();
    const int p = threadIdx.x;
    if (p < P && tile0 + p < n) {
        float density = v.average_init_density * expf(geo[p]);
        density = density * aux[p];
        const float alpha = 1.f - expf(-(density * delta));
        if (d_scratch != nullptr) d_scratch[tile0 + p] = alpha;
        if (d_alpha != nullptr) {
            if (HALF) reinterpret_cast<__half*>(d_alpha)[tile0 + p] = __float2half_rn(alpha);
            else reinterpret_cast<float*>(d_alpha)[tile0 + p] = alpha;
        }
        if (d_density != nullptr) d_density[tile0 + p] = density;
    }
    if (d_rgb == nullptr) return;
    __syncthreads();                                             // aux becomes the colour head's scale
    if (p < P) aux[p] = 1.f;
    hid = hidden_layers(v.color, v.color.n_extra, geo + P, X, H, wl);
    output_layer<HALF>(v.color, hid, X, wl, aux, d_rgb, tile0, n);
}

template <bool HALF>
__global__ __launch_bounds__(THREADS) void field_feature_kernel(const pixie_field_voxelize_desc v, const float* d_points, int64_t n,
                                                                const float* d_scratch, void* d_features) {
    extern __shared__ float lds[];
    float *X = lds + X_OFF, *H = lds + H_OFF, *wl = lds + WL_OFF, *pos = lds + POS_OFF, *aux = lds + AUX_OFF;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    tile_positions(v, d_points, tile0, n, false, pos, aux);
    const int p = threadIdx.x;
    if (p < P) aux[p] = (d_scratch != nullptr && tile0 + p < n) ? d_scratch[tile0 + p] : 1.f;
    __syncthreads();
    encode_tile(v.feature, pos, nullptr, tile0, n, X);
    const float* hid = hidden_layers(v.feature, input_width(v.feature), X, X, H, wl);
    output_layer<HALF>(v.feature, hid, X, wl, aux, d_features, tile0, n);
}

int check_desc(const pixie_hashmlp_desc* m, const char* what) {
    PX_REQUIRE(m != nullptr, "%s: null descriptor", what);
    PX_REQUIRE(m->n_levels >= 0 && m->n_levels <= PIXIE_HASHMLP_MAX_LEVELS, "%s: n_levels %d outside 0..%d", what, m->n_levels, PIXIE_HASHMLP_MAX_LEVELS);
    if (m->n_levels > 0) {
        PX_REQUIRE(m->features_per_level == 2 || m->features_per_level == 4 || m->features_per_level == 8,
                   "%s: features_per_level %d is not 2, 4 or 8", what, m->features_per_level);
        PX_REQUIRE(m->d_table != nullptr && (reinterpret_cast<uintptr_t>(m->d_table) & 15) == 0, "%s: d_table is null or not 16-byte aligned", what);
        for (int l = 0; l < m->n_levels; ++l) {
            const pixie_hashgrid_level& lv = m->level[l];
            PX_REQUIRE(lv.size > 0 && (int64_t)lv.offset + (int64_t)lv.size <= m->table_rows,
                       "%s: level %d (offset %u, size %u) does not fit the table of %lld rows", what, l, lv.offset, lv.size, (long long)m->table_rows);
            PX_REQUIRE(std::isfinite(lv.scale) && std::isfinite(lv.shift), "%s: level %d has a non-finite scale or shift", what, l);
        }
    }
    PX_REQUIRE(m->n_frequencies >= 0 && m->n_frequencies <= 8, "%s: n_frequencies %d outside 0..8", what, m->n_frequencies);
    PX_REQUIRE(m->n_extra >= 0 && m->n_extra <= PIXIE_HASHMLP_MAX_INPUT, "%s: n_extra %d outside 0..%d", what, m->n_extra, PIXIE_HASHMLP_MAX_INPUT);
    const int width = m->n_levels * (m->n_levels > 0 ? m->features_per_level : 0) + 6 * m->n_frequencies + m->n_extra;
    PX_REQUIRE(width >= 1 && width <= PIXIE_HASHMLP_MAX_INPUT, "%s: input row of %d columns outside 1..%d", what, width, PIXIE_HASHMLP_MAX_INPUT);
    PX_REQUIRE(m->n_hidden >= 1 && m->n_hidden <= PIXIE_HASHMLP_MAX_LAYERS - 1, "%s: %d hidden layers outside 1..%d (each 64 wide)", what, m->n_hidden,
               PIXIE_HASHMLP_MAX_LAYERS - 1);
    PX_REQUIRE(m->out_dim >= 1 && m->out_dim <= PIXIE_HASHMLP_MAX_OUTPUT, "%s: out_dim %d outside 1..%d", what, m->out_dim, PIXIE_HASHMLP_MAX_OUTPUT);
    PX_REQUIRE(m->out_activation >= 0 && m->out_activation <= 2, "%s: out_activation %d is not 0 (none), 1 (sigmoid) or 2 (exp)", what, m->out_activation);
    for (int i = 0; i <= m->n_hidden; ++i) PX_REQUIRE(m->d_weight[i] != nullptr, "%s: d_weight[%d] is null", what, i);
    return 0;
}

int check_field(const pixie_field_voxelize_desc* v, const char* what) {
    PX_REQUIRE(v != nullptr, "%s: null descriptor", what);
    if (check_desc(&v->density, "field query (density)") || check_desc(&v->color, "field query (color)") ||
        check_desc(&v->feature, "field query (feature)"))
        return 1;
    PX_REQUIRE(v->density.out_dim >= 2 && v->density.out_dim <= 63 && v->density.out_activation == 0 && v->density.n_extra == 0 && v->density.n_levels > 0,
               "%s: the density net must take positions alone and have 2..63 linear outputs (out_dim %d)", what, v->density.out_dim);
    PX_REQUIRE(v->color.n_levels == 0 && v->color.n_frequencies == 0 && v->color.n_extra == v->density.out_dim - 1 && v->color.out_dim == 3,
               "%s: the colour head must take the %d geometry columns alone and give 3 outputs", what, v->density.out_dim - 1);
    PX_REQUIRE(v->feature.n_extra == 0 && v->feature.n_levels > 0, "%s: the feature net takes positions alone", what);
    if (!v->contraction)
        for (int a = 0; a < 3; ++a) PX_REQUIRE(v->aabb[3 + a] > v->aabb[a], "%s: empty aabb on axis %d", what, a);
    return 0;
}

template <class K>
int prepare(K kern) {
    PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(kern)));
    return 0;
}

}  // namespace

extern "C" {

int pixie_hashmlp_forward(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, float* d_out, void* stream) {
    if (check_desc(desc, "pixie_hashmlp_forward")) return 1;
    PX_REQUIRE(n >= 0 && n <= (int64_t)0x7fffffff * P, "pixie_hashmlp_forward: n = %lld out of range", (long long)n);
    PX_REQUIRE(d_positions != nullptr || (desc->n_levels == 0 && desc->n_frequencies == 0), "pixie_hashmlp_forward: d_positions is null");
    PX_REQUIRE((d_extra != nullptr) == (desc->n_extra > 0) || n == 0, "pixie_hashmlp_forward: d_extra must be given iff n_extra > 0");
    if (n == 0) return 0;
    PX_REQUIRE(d_out != nullptr && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "pixie_hashmlp_forward: d_out is null or not 16-byte aligned");
    if (prepare(hashmlp_forward_kernel)) return 1;
    hipLaunchKernelGGL(hashmlp_forward_kernel, dim3((unsigned)cdiv(n, P)), dim3(THREADS), LDS_BYTES, as_stream(stream), *desc, d_positions, d_extra, n, d_out);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_field_voxelize(const pixie_field_voxelize_desc* v, void* d_features, void* d_alpha, void* d_rgb, float* d_density, float* d_scratch,
                         void* stream) {
    if (check_field(v, "pixie_field_voxelize")) return 1;
    PX_REQUIRE(v->d >= 1 && v->h >= 1 && v->w >= 1, "pixie_field_voxelize: empty lattice %d x %d x %d", v->d, v->h, v->w);
    PX_REQUIRE(std::isfinite(v->voxel_size) && v->voxel_size > 0, "pixie_field_voxelize: voxel_size must be positive");
    PX_REQUIRE((v->d_axis_x != nullptr) == (v->d_axis_y != nullptr) && (v->d_axis_x != nullptr) == (v->d_axis_z != nullptr),
               "pixie_field_voxelize: give all three axes or none");
    const int64_t n = (int64_t)v->d * v->h * v->w;
    PX_REQUIRE(d_features && d_alpha && d_rgb && d_scratch, "pixie_field_voxelize: null output or scratch pointer");
    PX_REQUIRE((reinterpret_cast<uintptr_t>(d_features) & 15) == 0, "pixie_field_voxelize: d_features is not 16-byte aligned");
    if (prepare(field_density_color_kernel<true>) || prepare(field_feature_kernel<true>)) return 1;
    const dim3 grid((unsigned)cdiv(n, P)), block(THREADS);
    hipLaunchKernelGGL(field_density_color_kernel<true>, grid, block, LDS_BYTES, as_stream(stream), *v, (const float*)nullptr, n, (float)v->voxel_size,
                       d_alpha, d_rgb, d_density, d_scratch);
    PX_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(field_feature_kernel<true>, grid, block, LDS_BYTES, as_stream(stream), *v, (const float*)nullptr, n,
                       v->alpha_weighted ? (const float*)d_scratch : (const float*)nullptr, d_features);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_field_query_points(const pixie_field_voxelize_desc* v, const float* d_world, int64_t n, double delta, float* d_features, float* d_alpha,
                             float* d_rgb, float* d_density, void* stream) {
    if (check_field(v, "pixie_field_query_points")) return 1;
    PX_REQUIRE(n >= 0 && n <= (int64_t)0x7fffffff * P, "pixie_field_query_points: n = %lld out of range", (long long)n);
    if (n == 0) return 0;
    PX_REQUIRE(d_world != nullptr, "pixie_field_query_points: d_world is null");
    PX_REQUIRE(d_features == nullptr || (reinterpret_cast<uintptr_t>(d_features) & 15) == 0, "pixie_field_query_points: d_features is not 16-byte aligned");
    const dim3 grid((unsigned)cdiv(n, P)), block(THREADS);
    if (d_alpha != nullptr || d_rgb != nullptr || d_density != nullptr) {
        if (prepare(field_density_color_kernel<false>)) return 1;
        hipLaunchKernelGGL(field_density_color_kernel<false>, grid, block, LDS_BYTES, as_stream(stream), *v, d_world, n, (float)delta, (void*)d_alpha,
                           (void*)d_rgb, d_density, (float*)nullptr);
        PX_CHECK_HIP(hipGetLastError());
    }
    if (d_features != nullptr) {
        if (prepare(field_feature_kernel<false>)) return 1;
        hipLaunchKernelGGL(field_feature_kernel<false>, grid, block, LDS_BYTES, as_stream(stream), *v, d_world, n, (const float*)nullptr, (void*)d_features);
        PX_CHECK_HIP(hipGetLastError());
    }
    return 0;
}

}  // extern "C"
