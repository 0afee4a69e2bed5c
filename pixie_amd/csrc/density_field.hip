// pixie_amd/csrc/density_field.hip -- the proposal density field: nerfstudio's HashMLPDensityField.get_density, fused, with gradients.
// What ProposalNetworkSampler.generate_ray_samples calls once per proposal level: a small hash grid, a 16-wide MLP, trunc_exp.
//
//   forward    a lane per point, grid-stride over tiles of 256 points; the weights are staged once per workgroup in LDS (first layer
//              transposed, [input][unit]) and read as broadcasts.  Per level the lane gathers its 8 corner rows (8 independent loads
//              in flight), blends them, and feeds the F features straight into the 16 hidden accumulators it keeps in registers: no
//              input row is materialised.  Front end and cells are hashgrid_math.h, layers and trunc_exp density_field_math.h.
//   backward   recomputes the forward from the positions (nothing is saved per point), then per lane dh -> dZ_1 -> dZ_0 -> dX on
//              fmaf chains.  dX of the grid columns and the masked unit positions leave for the scratch (channel-major); max |dX|
//              is an unsigned atomic max on the magnitude bits.
//   weights    dW = dZ^T In and db = dZ^T 1 per layer on v_mfma_f32_16x16x4_f32: a wave writes its 64 points' dZ (16 columns) and
//              the layer's input (16-column chunks) into its own LDS rows, reads them back transposed as the A and B operands, 4 points
//              per instruction, and keeps the 16 x 16 products in registers across the grid-stride loop.  The four waves' sums are
//              added in wave order: one partial per workgroup (= slab), summed in slab order by a second launch.  No float atomics.
//   table      hashgrid_table_grad.h's scatter and finalise, the kernels field_query_backward.hip launches: one lane per (point, level,
//              corner, feature), llrint(w_corner dX 2^s) added by a no-return 64-bit integer atomic, s from the device-side maximum; a
//              finalise launch rounds each accumulator once.  A point with selector 0 has dX = 0 exactly and issues no atomic.
// Built with -ffp-contract=off: cells, corner weights and the blend round as written; the layers are explicit fmaf.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"
#include "density_field_math.h"
#include "hashgrid_check.h"
#include "hashgrid_grad_math.h"
#include "hashgrid_math.h"
#include "hashgrid_table_grad.h"

namespace {

using namespace pixie;
typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int W = df::kWidth, THREADS = df::kThreads, ZP = W + 1;      // ZP: row pitch of a wave's [point][unit] LDS rows

struct NetLds {
    float w0t[df::kMaxInput * W];                // [k][j] = W0[j][k]; n_hidden == 0: w0t[k] = w_out[k]
    float w1t[W * W];                            // [k][j] = W1[j][k]
    float w1n[W * W];                            // [j][k], for W1^T dZ1
    float wo[W];
    float b0[W], b1[W];
    float bo;
};

inline int host_in_dim(const pixie_density_field_desc& m) { return m.n_levels * m.features_per_level; }

template <int NH>
__device__ inline void stage_weights(const pixie_density_field_desc& m, int in_dim, NetLds& s) {
    const int tid = threadIdx.x;
    if (NH == 0) {
        for (int k = tid; k < in_dim; k += THREADS) s.w0t[k] = m.d_weight[0][k];
    } else {
        for (int i = tid; i < W * in_dim; i += THREADS) {
            const int j = i / in_dim, k = i - j * in_dim;
            s.w0t[k * W + j] = m.d_weight[0][i];
        }
        if (NH == 2)
            for (int i = tid; i < W * W; i += THREADS) {
                const float v = m.d_weight[1][i];
                s.w1n[i] = v;
                s.w1t[(i & (W - 1)) * W + (i >> 4)] = v;
            }
        if (tid < W) {
            s.wo[tid] = m.d_weight[NH][tid];
            s.b0[tid] = m.d_bias[0] != nullptr ? m.d_bias[0][tid] : 0.f;
            s.b1[tid] = (NH == 2 && m.d_bias[1] != nullptr) ? m.d_bias[1][tid] : 0.f;
        }
    }
    if (tid == 0) s.bo = m.d_bias[NH] != nullptr ? m.d_bias[NH][0] : 0.f;
}

// nerf-frame (or world) position -> masked unit position; returns the selector
__device__ inline int front_end(const pixie_density_field_desc& m, const float* A, const float* src, float* p) {
    const float x[3] = {src[0], src[1], src[2]};
    const int sel = hg::unit_position(A, m.contraction, m.aabb, x, p);
    if (!sel) { p[0] = 0.f; p[1] = 0.f; p[2] = 0.f; }
    return sel;
}

__device__ inline void load_affine(const pixie_density_field_desc& m, float* A) {
    if (m.d_world_to_nerf != nullptr)
        for (int i = 0; i < 12; ++i) A[i] = m.d_world_to_nerf[i];
}

// One point's network at the masked unit position p: returns h; z0 / z1 receive the hidden pre-activations (NH >= 1 / NH == 2);
// SAVE: the input row also goes to xrow (this lane's LDS row).
template <int F, int NH, bool SAVE>
__device__ inline float eval_point(const pixie_density_field_desc& m, const NetLds& s, const float* p, float* z0, float* z1, float* xrow) {
    float acc[W];
    float h = s.bo;
    if (NH > 0) df::layer_seed(s.b0, acc);
    for (int l = 0; l < m.n_levels; ++l) {
        const hg::Level lv = hg::level_of(m.level[l]);
        const hg::Cell c = hg::cell_of(lv, p);
        float v[8][F];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float* row = m.d_table + (size_t)hg::corner_row_k(lv, c, k) * F;
            if (F == 2) {
                const float2 t = *reinterpret_cast<const float2*>(row);
                v[k][0] = t.x; v[k][1] = t.y;
            } else {
#pragma unroll
                for (int q = 0; q < F; q += 4) {
                    const float4 t = *reinterpret_cast<const float4*>(row + q);
                    v[k][q] = t.x; v[k][q + 1] = t.y; v[k][q + 2] = t.z; v[k][q + 3] = t.w;
                }
            }
        }
        float f[F];
#pragma unroll
        for (int i = 0; i < F; ++i) f[i] = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float wk = hg::corner_weight(c, k);
#pragma unroll
            for (int i = 0; i < F; ++i) f[i] += wk * v[k][i];
        }
#pragma unroll
        for (int i = 0; i < F; ++i) {
            const int col = l * F + i;
            if (SAVE) xrow[col] = f[i];
            if (NH == 0) h = fmaf(s.w0t[col], f[i], h);
            else df::layer_column(s.w0t + col * W, f[i], acc);
        }
    }
    if (NH == 0) return h;
    float a[W];
#pragma unroll
    for (int j = 0; j < W; ++j) { z0[j] = acc[j]; a[j] = df::relu(acc[j]); }
    if (NH == 2) {
        df::layer_seed(s.b1, acc);
#pragma unroll
        for (int k = 0; k < W; ++k) df::layer_column(s.w1t + k * W, a[k], acc);
#pragma unroll
        for (int j = 0; j < W; ++j) { z1[j] = acc[j]; a[j] = df::relu(acc[j]); }
    }
#pragma unroll
    for (int j = 0; j < W; ++j) h = fmaf(s.wo[j], a[j], h);
    return h;
}

// ---- forward ------------------------------------------------------------------------------------------------------------------
template <int F, int NH>
__global__ __launch_bounds__(THREADS) void density_forward_kernel(const pixie_density_field_desc m, const float* d_positions, int64_t n,
                                                                  float* d_density, float* d_raw) {
    __shared__ NetLds s;
    stage_weights<NH>(m, m.n_levels * F, s);
    float A[12];
    load_affine(m, A);
    __syncthreads();
    const int64_t tiles = df::tiles_of(n);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
        asm volatile("" ::: "memory");            // the staged weights are read where they are used, not hoisted into registers
        const int64_t pt = tile * THREADS + threadIdx.x;
        if (pt >= n) continue;
        float p[3];
        const int sel = front_end(m, m.d_world_to_nerf != nullptr ? A : nullptr, d_positions + 3 * pt, p);
        if (!sel) {
            d_density[pt] = 0.f;
            if (d_raw == nullptr) continue;
        }
        float z0[W], z1[W];
        const float h = eval_point<F, NH, false>(m, s, p, z0, z1, nullptr);
        if (d_raw != nullptr) d_raw[pt] = h;
        if (sel) d_density[pt] = df::density_of(h, m.average_init_density);
    }
}

// ---- backward -----------------------------------------------------------------------------------------------------------------
// acc[i][j] += sum over the wave's 64 points of a_rows[point][i] * b_rows[point][col0 + j] (b_rows null: * 1)
// v_mfma_f32_16x16x4_f32: lane l gives A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; register r holds D[4 (l >> 4) + r][l & 15]
__device__ inline f32x4 wave_product(const float* a_rows, const float* b_rows, int bp, int col0, f32x4 acc, int lane) {
    const int i = lane & 15, kq = lane >> 4;
#pragma unroll 4
    for (int t = 0; t < 16; ++t) {
        const float a = a_rows[(4 * t + kq) * ZP + i];
        const float b = b_rows != nullptr ? b_rows[(4 * t + kq) * bp + col0 + i] : 1.f;
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

__device__ inline f32x4 zero4() {
    f32x4 v = {0.f, 0.f, 0.f, 0.f};
    return v;
}

// dynamic LDS, per wave: zs [64][ZP] (the A operand: a layer's dZ) | hs [64][ZP] (a hidden layer's output) | xs [64][XP] (the input row,
// XP = 16 ceil(in_dim / 16) + 1, the columns past in_dim zero)
inline int x_pitch(int in_dim) { return 16 * ((in_dim + 15) / 16) + 1; }
constexpr int NET_FLOATS = (int)((sizeof(NetLds) + 15) / 16 * 4);        // the staged weights lead the dynamic LDS (a static block beside the
                                                                         // largest dynamic size the attribute allows would not fit)
inline size_t backward_lds_bytes(int in_dim) { return sizeof(float) * (NET_FLOATS + 4 * 64 * (size_t)(2 * ZP + x_pitch(in_dim))); }

template <int F, int NH>
__global__ __launch_bounds__(THREADS) void density_backward_kernel(const pixie_density_field_desc m, const float* d_positions, int64_t n,
                                                                   const float* d_ddensity, float* d_pos, float* d_dxg, float* d_part,
                                                                   unsigned int* d_max_bits) {
    extern __shared__ float lds[];
    NetLds& s = *reinterpret_cast<NetLds*>(lds);
    float* dyn = lds + NET_FLOATS;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int in_dim = m.n_levels * F, C0 = (in_dim + 15) / 16, XP = 16 * C0 + 1, per_wave = 64 * (2 * ZP + XP);
    float* zs = dyn + wave * per_wave;
    float* hs = zs + 64 * ZP;
    float* xs = hs + 64 * ZP;
    stage_weights<NH>(m, in_dim, s);
    for (int i = tid; i < 4 * per_wave; i += THREADS) dyn[i] = 0.f;
    float A[12];
    load_affine(m, A);
    __syncthreads();

    f32x4 accX[4] = {zero4(), zero4(), zero4(), zero4()};
    f32x4 accXb = zero4(), acc1 = zero4(), acc1b = zero4(), accO = zero4(), accOb = zero4();
    unsigned int mx = 0;
    float* zrow = zs + lane * ZP;
    float* hrow = hs + lane * ZP;
    float* xrow = xs + lane * XP;
    const int64_t tiles = df::tiles_of(n);
    for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {             // the trip count is the workgroup's: barriers inside
        asm volatile("" ::: "memory");            // as in the forward
        const int64_t pt = tile * THREADS + tid;
        const bool inside = pt < n;
        float p[3] = {0.f, 0.f, 0.f};
        int sel = 0;
        if (inside) sel = front_end(m, m.d_world_to_nerf != nullptr ? A : nullptr, d_positions + 3 * pt, p);
        float z0[W], z1[W];
#pragma unroll
        for (int j = 0; j < W; ++j) { z0[j] = 0.f; z1[j] = 0.f; }
        float h = 0.f;
        if (sel) h = eval_point<F, NH, true>(m, s, p, z0, z1, xrow);
        else for (int k = 0; k < in_dim; ++k) xrow[k] = 0.f;
        const float dh = sel ? df::dh_of(d_ddensity[pt], h, m.average_init_density, 1) : 0.f;

        float dz0[W];                             // dL/dZ of the first hidden layer (NH >= 1)
        if (NH == 0) {
#pragma unroll
            for (int j = 0; j < W; ++j) zrow[j] = j == 0 ? dh : 0.f;
            __syncthreads();
            for (int c = 0; c < 4; ++c)
                if (c < C0) accX[c] = wave_product(zs, xs, XP, 16 * c, accX[c], lane);
            accXb = wave_product(zs, nullptr, 0, 0, accXb, lane);
        } else {
            const float* zl = NH == 2 ? z1 : z0;
            float dzl[W];
#pragma unroll
            for (int j = 0; j < W; ++j) {
                dzl[j] = zl[j] > 0.f ? s.wo[j] * dh : 0.f;
                zrow[j] = j == 0 ? dh : 0.f;
                hrow[j] = df::relu(zl[j]);
            }
            __syncthreads();
            accO = wave_product(zs, hs, ZP, 0, accO, lane);
            accOb = wave_product(zs, nullptr, 0, 0, accOb, lane);
            if (NH == 2) {
                __syncthreads();
#pragma unroll
                for (int j = 0; j < W; ++j) { zrow[j] = dzl[j]; hrow[j] = df::relu(z0[j]); }
                __syncthreads();
                acc1 = wave_product(zs, hs, ZP, 0, acc1, lane);
                acc1b = wave_product(zs, nullptr, 0, 0, acc1b, lane);
                float dh0[W];
#pragma unroll
                for (int k = 0; k < W; ++k) dh0[k] = 0.f;
#pragma unroll
                for (int j = 0; j < W; ++j)
#pragma unroll
                    for (int k = 0; k < W; ++k) dh0[k] = fmaf(s.w1n[j * W + k], dzl[j], dh0[k]);
#pragma unroll
                for (int k = 0; k < W; ++k) dz0[k] = z0[k] > 0.f ? dh0[k] : 0.f;
            } else {
#pragma unroll
                for (int j = 0; j < W; ++j) dz0[j] = dzl[j];
            }
            __syncthreads();
#pragma unroll
            for (int j = 0; j < W; ++j) zrow[j] = dz0[j];
            __syncthreads();
            for (int c = 0; c < 4; ++c)
                if (c < C0) accX[c] = wave_product(zs, xs, XP, 16 * c, accX[c], lane);
            accXb = wave_product(zs, nullptr, 0, 0, accXb, lane);
        }
        if (d_dxg != nullptr && inside) {
            for (int col = 0; col < in_dim; ++col) {
                float dx = 0.f;
                if (sel) {
                    if (NH == 0) dx = s.w0t[col] * dh;
                    else {
#pragma unroll
                        for (int j = 0; j < W; ++j) dx = fmaf(s.w0t[col * W + j], dz0[j], dx);
                    }
                }
                d_dxg[(int64_t)col * n + pt] = dx;
                const unsigned int b = hgg::magnitude_bits(dx);
                mx = b > mx ? b : mx;
            }
#pragma unroll
            for (int a = 0; a < 3; ++a) d_pos[(int64_t)a * n + pt] = p[a];
        }
        __syncthreads();                          // the rows are read; the next tile overwrites them
    }
    if (d_dxg != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned int o = (unsigned int)__shfl_xor((int)mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0 && mx != 0) atomicMax(d_max_bits, mx);
    }

    // the wave's sums in the partial's layout (density_field_math.h), then the four waves in wave order
    const int pc = df::param_count(in_dim, NH), di = 4 * (lane >> 4), dj = lane & 15;
    float* wp = dyn + wave * per_wave;
    if (NH == 0) {
        if (lane < 16) {
            for (int c = 0; c < 4; ++c)
                if (c < C0 && 16 * c + dj < in_dim) wp[16 * c + dj] = accX[c][0];
            if (lane == 0) wp[in_dim] = accXb[0];
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            for (int c = 0; c < 4; ++c)
                if (c < C0 && 16 * c + dj < in_dim) wp[(di + r) * in_dim + 16 * c + dj] = accX[c][r];
            if (dj == 0) wp[W * in_dim + di + r] = accXb[r];
            if (NH == 2) {
                const int base1 = df::weight_offset(in_dim, NH, 1);
                wp[base1 + (di + r) * W + dj] = acc1[r];
                if (dj == 0) wp[base1 + W * W + di + r] = acc1b[r];
            }
        }
        const int baseO = df::weight_offset(in_dim, NH, NH);
        if (lane < 16) wp[baseO + dj] = accO[0];
        if (lane == 0) wp[baseO + W] = accOb[0];
    }
    __syncthreads();
    for (int e = tid; e < pc; e += THREADS)
        d_part[(int64_t)blockIdx.x * pc + e] = ((dyn[e] + dyn[per_wave + e]) + dyn[2 * per_wave + e]) + dyn[3 * per_wave + e];
}

// partial e of every slab, added in slab order (16 loads in flight), to the gradient it belongs to
__global__ void density_slab_sum_kernel(const float* d_part, int slabs, int in_dim, int n_hidden, const pixie_density_field_grads g) {
    const int e = blockIdx.x * blockDim.x + threadIdx.x, pc = df::param_count(in_dim, n_hidden);
    if (e >= pc) return;
    float* dst = nullptr;
    for (int i = 0; i <= n_hidden; ++i) {
        const int at = df::weight_offset(in_dim, n_hidden, i), cnt = df::layer_out(n_hidden, i) * df::layer_in(in_dim, i), out = df::layer_out(n_hidden, i);
        if (e >= at && e < at + cnt) dst = g.d_weight[i] != nullptr ? g.d_weight[i] + (e - at) : nullptr;
        else if (e >= at + cnt && e < at + cnt + out) dst = g.d_bias[i] != nullptr ? g.d_bias[i] + (e - at - cnt) : nullptr;
    }
    if (dst == nullptr) return;
    float sum = 0.f;
    int j = 0;
    for (; j + 16 <= slabs; j += 16) {
        float v[16];
#pragma unroll
        for (int u = 0; u < 16; ++u) v[u] = d_part[(int64_t)(j + u) * pc + e];
#pragma unroll
        for (int u = 0; u < 16; ++u) sum = sum + v[u];
    }
    for (; j < slabs; ++j) sum = sum + d_part[(int64_t)j * pc + e];
    *dst = sum;
}

// ---- table gradient -----------------------------------------------------------------------------------------------------------
// hashgrid_table_grad.h's scatter at the masked unit positions the backward wrote: d_pos [3][n]; d_dxg [in_dim][n]
__global__ __launch_bounds__(THREADS) void density_table_scatter_kernel(const pixie_density_field_desc m, const float* d_pos, int64_t n,
                                                                        const float* d_dxg, const unsigned int* d_header, unsigned long long* d_acc) {
    table_scatter_item(m, [d_pos, n](int64_t point, float* pp) {
        pp[0] = d_pos[point]; pp[1] = d_pos[n + point]; pp[2] = d_pos[2 * n + point];
    }, n, d_dxg, d_header, d_acc, THREADS);
}

// ---- host ---------------------------------------------------------------------------------------------------------------------
int check_desc(const pixie_density_field_desc* m, int64_t n, const char* what) {
    PX_REQUIRE(m != nullptr, "%s: null descriptor", what);
    PX_REQUIRE(m->hidden_width == PIXIE_DENSITY_FIELD_WIDTH, "%s: hidden_width %d is not %d (wider networks: pixie_hashmlp_forward)", what,
               m->hidden_width, PIXIE_DENSITY_FIELD_WIDTH);
    PX_REQUIRE(m->n_levels >= 1 && m->n_levels <= PIXIE_HASHMLP_MAX_LEVELS, "%s: n_levels %d outside 1..%d", what, m->n_levels, PIXIE_HASHMLP_MAX_LEVELS);
    PX_REQUIRE(m->features_per_level == 2 || m->features_per_level == 4 || m->features_per_level == 8, "%s: features_per_level %d is not 2, 4 or 8",
               what, m->features_per_level);
    PX_REQUIRE(host_in_dim(*m) <= PIXIE_DENSITY_FIELD_MAX_INPUT, "%s: input row of %d columns, at most %d", what, host_in_dim(*m),
               PIXIE_DENSITY_FIELD_MAX_INPUT);
    PX_REQUIRE(m->n_hidden >= 0 && m->n_hidden <= df::kMaxHidden, "%s: %d hidden layers outside 0..%d", what, m->n_hidden, df::kMaxHidden);
    if (check_grid_table(*m, what)) return 1;
    for (int i = 0; i <= m->n_hidden; ++i) PX_REQUIRE(m->d_weight[i] != nullptr, "%s: d_weight[%d] is null", what, i);
    if (!m->contraction)
        for (int a = 0; a < 3; ++a)
            PX_REQUIRE(m->aabb[3 + a] > m->aabb[a], "%s: empty aabb on axis %d (%g .. %g) and no contraction", what, a, (double)m->aabb[a],
                       (double)m->aabb[3 + a]);
    PX_REQUIRE(std::isfinite(m->average_init_density), "%s: average_init_density is not finite", what);
    PX_REQUIRE(n >= 0 && n <= df::kMaxPoints, "%s: n = %lld outside 0..2^24", what, (long long)n);
    return 0;
}

#define DF_DISPATCH(KERNEL, F_, NH_, ...)                                        \
    do {                                                                          \
        if ((F_) == 2 && (NH_) == 0) { KERNEL(2, 0, __VA_ARGS__); }               \
        else if ((F_) == 2 && (NH_) == 1) { KERNEL(2, 1, __VA_ARGS__); }          \
        else if ((F_) == 2) { KERNEL(2, 2, __VA_ARGS__); }                        \
        else if ((F_) == 4 && (NH_) == 0) { KERNEL(4, 0, __VA_ARGS__); }          \
        else if ((F_) == 4 && (NH_) == 1) { KERNEL(4, 1, __VA_ARGS__); }          \
        else if ((F_) == 4) { KERNEL(4, 2, __VA_ARGS__); }                        \
        else if ((NH_) == 0) { KERNEL(8, 0, __VA_ARGS__); }                       \
        else if ((NH_) == 1) { KERNEL(8, 1, __VA_ARGS__); }                       \
        else { KERNEL(8, 2, __VA_ARGS__); }                                       \
    } while (0)

#define DF_LAUNCH_FORWARD(F_, NH_, grid, st, ...) \
    hipLaunchKernelGGL((density_forward_kernel<F_, NH_>), grid, dim3(THREADS), 0, st, __VA_ARGS__)

#define DF_LAUNCH_BACKWARD(F_, NH_, grid, lds, st, ...)                                                                       \
    do {                                                                                                                       \
        PX_CHECK_HIP(allow_max_dynamic_lds(reinterpret_cast<const void*>(&density_backward_kernel<F_, NH_>)));                 \
        hipLaunchKernelGGL((density_backward_kernel<F_, NH_>), grid, dim3(THREADS), lds, st, __VA_ARGS__);                     \
    } while (0)

}  // namespace

extern "C" {

int pixie_density_field_train_bytes(const pixie_density_field_desc* desc, int64_t n, int64_t* saved_bytes, int64_t* scratch_bytes) {
    if (check_desc(desc, n, "pixie_density_field_train_bytes")) return 1;
    const df::Scratch L = df::scratch_layout(n, host_in_dim(*desc), desc->n_hidden, desc->table_rows, desc->features_per_level);
    if (saved_bytes != nullptr) *saved_bytes = df::saved_bytes(n);
    if (scratch_bytes != nullptr) *scratch_bytes = L.total;
    return 0;
}

int pixie_density_field_forward(const pixie_density_field_desc* desc, const float* d_positions, int64_t n, float* d_density, float* d_raw,
                                void* stream) {
    const char* what = "pixie_density_field_forward";
    if (check_desc(desc, n, what)) return 1;
    if (n == 0) return 0;
    PX_REQUIRE(d_positions != nullptr && d_density != nullptr, "%s: d_positions or d_density is null", what);
    const dim3 grid((unsigned)df::forward_blocks(n));
    hipStream_t st = as_stream(stream);
    DF_DISPATCH(DF_LAUNCH_FORWARD, desc->features_per_level, desc->n_hidden, grid, st, *desc, d_positions, n, d_density, d_raw);
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_density_field_backward(const pixie_density_field_desc* desc, const float* d_positions, int64_t n, const float* d_ddensity,
                                 const pixie_density_field_grads* grads, void* d_scratch, void* stream) {
    const char* what = "pixie_density_field_backward";
    if (check_desc(desc, n, what)) return 1;
    PX_REQUIRE(grads != nullptr, "%s: grads is null", what);
    const pixie_density_field_desc& m = *desc;
    const int F = m.features_per_level, in_dim = host_in_dim(m), NH = m.n_hidden;
    for (int i = NH + 1; i < PIXIE_DENSITY_FIELD_MAX_LAYERS; ++i)
        PX_REQUIRE(grads->d_weight[i] == nullptr && grads->d_bias[i] == nullptr, "%s: gradient pointer for layer %d of %d", what, i, NH + 1);
    bool any_layer = false;
    for (int i = 0; i <= NH; ++i) any_layer = any_layer || grads->d_weight[i] != nullptr || grads->d_bias[i] != nullptr;
    if (!any_layer && grads->d_table == nullptr) return 0;
    hipStream_t st = as_stream(stream);
    if (n == 0)
        return zero_empty_grads(*grads, NH + 1, (size_t)m.table_rows * F, [=](int i) { return std::make_pair(df::layer_out(NH, i), df::layer_in(in_dim, i)); }, st);
    PX_REQUIRE(d_positions != nullptr && d_ddensity != nullptr, "%s: d_positions or d_ddensity is null", what);
    PX_REQUIRE(d_scratch != nullptr && (reinterpret_cast<uintptr_t>(d_scratch) & 255) == 0, "%s: d_scratch is null or not 256-byte aligned", what);
    const df::Scratch L = df::scratch_layout(n, in_dim, NH, m.table_rows, F);
    char* base = reinterpret_cast<char*>(d_scratch);
    unsigned int* header = reinterpret_cast<unsigned int*>(base);
    float* pos = reinterpret_cast<float*>(base + L.pos);
    float* dxg = reinterpret_cast<float*>(base + L.dxg);
    float* part = reinterpret_cast<float*>(base + L.part);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + L.acc);
    const bool table = grads->d_table != nullptr;
    const int slabs = df::slab_count(n);

    PX_CHECK_HIP(hipMemsetAsync(header, 0, df::kHeaderBytes, st));
    if (table) PX_CHECK_HIP(hipMemsetAsync(acc, 0, 8 * (size_t)m.table_rows * F, st));
    const dim3 grid((unsigned)slabs);
    const size_t lds = backward_lds_bytes(in_dim);
    DF_DISPATCH(DF_LAUNCH_BACKWARD, F, NH, grid, lds, st, m, d_positions, n, d_ddensity, pos, table ? dxg : (float*)nullptr, part, header);
    PX_CHECK_HIP(hipGetLastError());
    if (any_layer) {
        const int pc = df::param_count(in_dim, NH);
        hipLaunchKernelGGL(density_slab_sum_kernel, dim3((unsigned)cdiv(pc, 64)), dim3(64), 0, st, (const float*)part, slabs, in_dim, NH, *grads);
        PX_CHECK_HIP(hipGetLastError());
    }
    if (table) return finish_table_grad(density_table_scatter_kernel, THREADS, m, pos, n, dxg, header, acc, grads->d_table, st);
    return 0;
}

}  // extern "C"
