// pixie_amd/csrc/field_query_backward.hip -- the hash-grid MLP of field_query.hip with gradients: what tiny-cuda-nn's
// NetworkWithInputEncoding gives the F3RM model under torch.autograd (nerfacto_field.py, f3rm/feature_field.py:71-82).
//
//   forward_saved   field_query_body.h's tile body, call for call, so d_out carries pixie_hashmlp_forward's bits; after the encoding and
//                   after every hidden layer the LDS rows also leave for d_saved, channel-major ([column][n]): a tile's 64 points are 256
//                   contiguous bytes of every column, and the LDS reads run along the point axis, conflict-free.
//   backward tile   one workgroup per 64 points.  dH_last = W_out^T dZ_out with dZ_out = dY act'(Y) formed on load and streamed in
//                   64-column chunks; then dZ_k = dH_k [H_k > 0], dH_(k-1) = W_k^T dZ_k down to dX = W_0^T dZ_0.  Each product is
//                   the forward's W[64][K] X[K][64] shape on v_mfma_f32_32x32x2_f32 with the weight chunk staged as it lies in memory
//                   (wl[out][in]: the forward stages the transpose).  dZ_k, the grid columns of dX (both channel-major) and d_extra go
//                   to HBM; max |dX_grid| is reduced by an unsigned atomic max on the magnitude bits (exact, order-free, NaN above Inf).
//   weights         dW = dZ^T A and db = sum dZ over a fixed slab of points per workgroup on the same instruction; slab partials are
//                   written and summed in slab order by a second launch: no float atomics.
//   table           one lane per (point, level, corner, feature): consecutive lanes are the F features of one row (F x 8 contiguous
//                   bytes of accumulators), consecutive groups the 8 corners of one cell (x neighbours are adjacent rows on dense
//                   levels).  c = w_corner dX[column] in float32, llrint(c 2^s) added by a no-return 64-bit integer atomic; the shift
//                   s comes from the device-side maximum (hashgrid_grad_math.h).  A finalise launch rounds each accumulator once.
// Built with -ffp-contract=off like field_query.hip: cells and corner weights round as the forward's.
#include "field_query_body.h"
#include "hashgrid_grad_math.h"
#include "hashgrid_table_grad.h"
#include "hashmlp_plan.h"

namespace {

constexpr int ZLD = 65;                          // row pitch of the staged gradient chunk [row][point or column]

// ---- training forward ---------------------------------------------------------------------------------------------------------
// rows [rows][P] of LDS -> dst[row][n] at the tile's points
__device__ inline void save_rows(const float* src, int rows, float* dst, int64_t tile0, int64_t n) {
    for (int i = threadIdx.x; i < rows * P; i += THREADS) {
        const int c = i >> 6, p = i & (P - 1);
        if (tile0 + p < n) dst[(int64_t)c * n + tile0 + p] = src[c * P + p];
    }
}

__global__ __launch_bounds__(THREADS) void hashmlp_forward_saved_kernel(const pixie_hashmlp_desc m, const float* d_positions, const float* d_extra,
                                                                        int64_t n, float* d_out, float* d_saved) {
    extern __shared__ float lds[];
    float *X = lds + X_OFF, *H = lds + H_OFF, *wl = lds + WL_OFF, *pos = lds + POS_OFF;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    load_tile_positions(d_positions, tile0, n, pos);
    encode_tile(m, pos, d_extra, tile0, n, X);
    const int in_dim = hg::input_width(m);
    __syncthreads();
    save_rows(X, in_dim, d_saved, tile0, n);
    float* hidden = d_saved + (int64_t)in_dim * n;
    const float* src = X;
    for (int i = 0; i < m.n_hidden; ++i) {        // hidden_layers(), with the rows leaving after each layer (as a per-layer hook of
                                                  // hidden_layers the same lines compile to other device code)
        float* dst = (src >= H && src < H + 64 * P) ? X : H;
        lds_layer(m.d_weight[i], m.d_bias[i], 64, i == 0 ? in_dim : 64, true, src, dst, wl);
        __syncthreads();
        save_rows(dst, 64, hidden + (int64_t)i * 64 * n, tile0, n);
        src = dst;
    }
    output_layer<false>(m, src, X, wl, nullptr, d_out, tile0, n);
}

// ---- backward tile ------------------------------------------------------------------------------------------------------------
__device__ inline void store_weights_natural(const float (&v)[WPT], float* wl) {      // wl[out][in], as load_weights read them
#pragma unroll
    for (int j = 0; j < WPT; ++j) {
        const int i = threadIdx.x + j * THREADS, k = i & 63, o = i >> 6;
        wl[o * WLD + k] = v[j];
    }
}

// acc[row][point] += sum over the chunk's 64 k of wl[k][row] b[k][point]; b: LDS rows of pitch `ld`
__device__ inline f32x16 chunk_product(const float* wl, const float* b, int ld, f32x16 acc, int mb, int nb, int r, int hi) {
#pragma unroll 8
    for (int kp = 0; kp < 32; ++kp) {
        const float a = wl[(2 * kp + hi) * WLD + mb * 32 + r];
        const float x = b[(2 * kp + hi) * ld + nb * 32 + r];
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, x, acc, 0, 0, 0);
    }
    return acc;
}

__device__ inline f32x16 zero_acc() {
    f32x16 acc;
#pragma unroll
    for (int g = 0; g < 16; ++g) acc[g] = 0.f;
    return acc;
}

__device__ inline float act_derivative(float dy, float y, int act) {
    if (act == 1) return dy * (y * (1.f - y));
    if (act == 2) return dy * y;
    return dy;
}

// d_dz: [n_hidden][64][n]; d_dxg: [levels * F][n] or null; d_dextra: (n, n_extra) or null
__global__ __launch_bounds__(THREADS) void hashmlp_backward_kernel(const pixie_hashmlp_desc m, int64_t n, const float* d_out, const float* d_dout,
                                                                   const float* d_saved, float* d_dz, float* d_dxg, float* d_dextra,
                                                                   unsigned int* d_max_bits) {
    __shared__ float G0[64 * P];
    __shared__ float G1[64 * ZLD];               // the dY chunk of the output layer, then the second gradient buffer
    __shared__ float wl[64 * WLD];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hi = lane >> 5, mb = wave & 1, nb = wave >> 1;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    const int in_dim = hg::input_width(m), out_dim = m.out_dim, act = m.out_activation;
    const float* hidden = d_saved + (int64_t)in_dim * n;
    const int64_t gp = tile0 + nb * 32 + r;       // the point of this lane's accumulator column

    // dH of the last hidden layer: sum over the outputs, 64 at a time
    f32x16 acc = zero_acc();
    {
        const float* W = m.d_weight[m.n_hidden];
        float wv[WPT], dv[WPT];
        for (int o0 = 0; o0 < out_dim; o0 += 64) {
            load_weights(W, out_dim, 64, o0, 0, wv);
#pragma unroll
            for (int j = 0; j < WPT; ++j) {
                const int i = tid + j * THREADS, o = i & 63, p = i >> 6;
                float v = 0.f;
                if (tile0 + p < n && o0 + o < out_dim) {
                    const int64_t at = (tile0 + p) * out_dim + o0 + o;
                    v = d_dout[at];
                    if (act != 0) v = act_derivative(v, d_out[at], act);
                }
                dv[j] = v;
            }
            __syncthreads();                      // the previous chunk has been multiplied
            store_weights_natural(wv, wl);
#pragma unroll
            for (int j = 0; j < WPT; ++j) {
                const int i = tid + j * THREADS, o = i & 63, p = i >> 6;
                G1[o * ZLD + p] = dv[j];
            }
            __syncthreads();
            acc = chunk_product(wl, G1, ZLD, acc, mb, nb, r, hi);
        }
        __syncthreads();                          // G1 becomes a gradient buffer
    }

    for (int k = m.n_hidden - 1; k >= 0; --k) {
        float* G = (k & 1) ? G1 : G0;
        const float* Hk = hidden + (int64_t)k * 64 * n;
        float* dzk = d_dz + (int64_t)k * 64 * n;
#pragma unroll
        for (int g = 0; g < 16; ++g) {
            const int h = mb * 32 + acc_row(g, hi);
            float v = 0.f;
            if (gp < n) {
                v = Hk[(int64_t)h * n + gp] > 0.f ? acc[g] : 0.f;
                dzk[(int64_t)h * n + gp] = v;
            }
            G[h * P + nb * 32 + r] = v;
        }
        if (k == 0) break;
        float wv[WPT];
        load_weights(m.d_weight[k], 64, 64, 0, 0, wv);
        __syncthreads();                          // G is complete; wl has been read
        store_weights_natural(wv, wl);
        __syncthreads();
        acc = chunk_product(wl, G, P, zero_acc(), mb, nb, r, hi);
    }

    if (d_dxg == nullptr && d_dextra == nullptr) return;
    const int n_grid = m.n_levels * m.features_per_level, extra0 = n_grid + 6 * m.n_frequencies;
    unsigned int mx = 0;
    for (int c0 = 0; c0 < in_dim; c0 += 64) {
        const bool grid_part = d_dxg != nullptr && c0 < n_grid, extra_part = d_dextra != nullptr && c0 + 64 > extra0;
        if (!grid_part && !extra_part) continue;  // frequency columns have no parameters: their dX is dropped
        float wv[WPT];
        load_weights(m.d_weight[0], 64, in_dim, 0, c0, wv);
        __syncthreads();                          // G0 is complete; wl has been read
        store_weights_natural(wv, wl);
        __syncthreads();
        acc = chunk_product(wl, G0, P, zero_acc(), mb, nb, r, hi);
        if (gp < n) {
#pragma unroll
            for (int g = 0; g < 16; ++g) {
                const int c = c0 + mb * 32 + acc_row(g, hi);
                if (c < n_grid) {
                    if (d_dxg != nullptr) {
                        d_dxg[(int64_t)c * n + gp] = acc[g];
                        const unsigned int b = hgg::magnitude_bits(acc[g]);
                        mx = b > mx ? b : mx;
                    }
                } else if (c >= extra0 && c < in_dim && d_dextra != nullptr) {
                    d_dextra[gp * m.n_extra + (c - extra0)] = acc[g];
                }
            }
        }
    }
    if (d_dxg != nullptr) {
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) {
            const unsigned int o = (unsigned int)__shfl_xor((int)mx, off, 64);
            mx = o > mx ? o : mx;
        }
        if (lane == 0 && mx != 0) atomicMax(d_max_bits, mx);
    }
}

// ---- weight and bias gradients ------------------------------------------------------------------------------------------------
// part[slab][o][k] = sum over the slab's points of dZ[p][o] A[p][k]; bpart[slab][o] = sum dZ[p][o].
// OUT: Z is dY (n, O) row-major, multiplied by the activation derivative from Y on load; otherwise Z is [O][n].  A is [K][n].
template <bool OUT>
__global__ __launch_bounds__(THREADS) void weight_grad_kernel(const float* Z, const float* Y, int act, const float* A, int64_t n, int O, int K,
                                                              int k_tiles, int64_t chunks_per_slab, float* part, float* bpart) {
    __shared__ float zs[64 * ZLD];               // [point][o]
    __shared__ float as[64 * ZLD];               // [point][k]
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, r = lane & 31, hi = lane >> 5, mb = wave & 1, nb = wave >> 1;
    const int o0 = ((int)blockIdx.x / k_tiles) * 64, k0 = ((int)blockIdx.x % k_tiles) * 64, slab = blockIdx.y;
    const int64_t tiles = (n + P - 1) / P, first = slab * chunks_per_slab;
    const int64_t last = first + chunks_per_slab < tiles ? first + chunks_per_slab : tiles;
    f32x16 acc = zero_acc();
    float bsum = 0.f;
    float zv[WPT], av[WPT];
    // one chunk of 64 points into registers: 32 loads per thread in flight together, and, from the second chunk on, under the matrix work
    auto load_chunk = [&](int64_t p0) {
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = tid + j * THREADS, lo = i & 63, up = i >> 6;
            float v = 0.f;
            if (OUT) {                            // lo: output column, up: point
                if (p0 + up < n && o0 + lo < O) {
                    const int64_t at = (p0 + up) * O + o0 + lo;
                    v = Z[at];
                    if (act != 0) v = act_derivative(v, Y[at], act);
                }
            } else if (p0 + lo < n && o0 + up < O) {          // lo: point, up: row
                v = Z[(int64_t)(o0 + up) * n + p0 + lo];
            }
            zv[j] = v;
            av[j] = (p0 + lo < n && k0 + up < K) ? A[(int64_t)(k0 + up) * n + p0 + lo] : 0.f;
        }
    };
    if (first < last) load_chunk(first * P);
    for (int64_t t = first; t < last; ++t) {
        __syncthreads();                          // the previous chunk has been multiplied
#pragma unroll
        for (int j = 0; j < WPT; ++j) {
            const int i = tid + j * THREADS, lo = i & 63, up = i >> 6;
            if (OUT) zs[up * ZLD + lo] = zv[j]; else zs[lo * ZLD + up] = zv[j];
            as[lo * ZLD + up] = av[j];
        }
        __syncthreads();
        if (t + 1 < last) load_chunk((t + 1) * P);
#pragma unroll 8
        for (int kp = 0; kp < 32; ++kp) {
            const float a = zs[(2 * kp + hi) * ZLD + mb * 32 + r];
            const float b = as[(2 * kp + hi) * ZLD + nb * 32 + r];
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        if (k0 == 0 && tid < 64)
            for (int p = 0; p < P; ++p) bsum = bsum + zs[p * ZLD + tid];
    }
#pragma unroll
    for (int g = 0; g < 16; ++g) {
        const int o = o0 + mb * 32 + acc_row(g, hi), k = k0 + nb * 32 + r;
        if (o < O && k < K) part[((int64_t)slab * O + o) * K + k] = acc[g];
    }
    if (k0 == 0 && tid < 64 && o0 + tid < O) bpart[(int64_t)slab * O + o0 + tid] = bsum;
}

__global__ void slab_sum_kernel(const float* part, const float* bpart, int slabs, int O, int K, float* dW, float* db) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x, ok = O * K;
    if (i < ok) {
        if (dW == nullptr) return;
        float s = 0.f;
        int j = 0;
        for (; j + 8 <= slabs; j += 8) {          // eight loads in flight; the additions stay in slab order
            float v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) v[u] = part[(int64_t)(j + u) * ok + i];
#pragma unroll
            for (int u = 0; u < 8; ++u) s = s + v[u];
        }
        for (; j < slabs; ++j) s = s + part[(int64_t)j * ok + i];
        dW[i] = s;
    } else if (i < ok + O && db != nullptr) {
        float s = 0.f;
        for (int j = 0; j < slabs; ++j) s = s + bpart[(int64_t)j * O + (i - ok)];
        db[i - ok] = s;
    }
}

// ---- table gradient -----------------------------------------------------------------------------------------------------------
// hashgrid_table_grad.h's scatter at the unit-cube positions the forward took
__global__ __launch_bounds__(THREADS) void table_scatter_kernel(const pixie_hashmlp_desc m, const float* d_positions, int64_t n, const float* d_dxg,
                                                                const unsigned int* d_header, unsigned long long* d_acc) {
    table_scatter_item(m, [d_positions](int64_t point, float* pp) {
        pp[0] = d_positions[3 * point]; pp[1] = d_positions[3 * point + 1]; pp[2] = d_positions[3 * point + 2];
    }, n, d_dxg, d_header, d_acc, THREADS);
}

int check_call(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, const char* what) {
    if (check_desc(desc, what)) return 1;
    PX_REQUIRE(n >= 0 && n <= hgg::kMaxPoints, "%s: n = %lld outside 0..2^24", what, (long long)n);
    PX_REQUIRE(d_positions != nullptr || (desc->n_levels == 0 && desc->n_frequencies == 0), "%s: d_positions is null", what);
    PX_REQUIRE((d_extra != nullptr) == (desc->n_extra > 0) || n == 0, "%s: d_extra must be given iff n_extra > 0", what);
    return 0;
}

}  // namespace

extern "C" {

int pixie_hashmlp_train_bytes(const pixie_hashmlp_desc* desc, int64_t n, int64_t* saved_bytes, int64_t* scratch_bytes) {
    if (check_desc(desc, "pixie_hashmlp_train_bytes")) return 1;
    PX_REQUIRE(n >= 0 && n <= hgg::kMaxPoints, "pixie_hashmlp_train_bytes: n = %lld outside 0..2^24", (long long)n);
    if (saved_bytes != nullptr) *saved_bytes = hmp::saved_bytes(*desc, n);
    if (scratch_bytes != nullptr) *scratch_bytes = hmp::scratch_layout(*desc, n).total;
    return 0;
}

int pixie_hashmlp_forward_saved(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, float* d_out,
                                void* d_saved, void* stream) {
    if (check_call(desc, d_positions, d_extra, n, "pixie_hashmlp_forward_saved")) return 1;
    if (n == 0) return 0;
    PX_REQUIRE(d_out != nullptr && (reinterpret_cast<uintptr_t>(d_out) & 15) == 0, "pixie_hashmlp_forward_saved: d_out is null or not 16-byte aligned");
    PX_REQUIRE(d_saved != nullptr && (reinterpret_cast<uintptr_t>(d_saved) & 3) == 0, "pixie_hashmlp_forward_saved: d_saved is null or misaligned");
    if (prepare(hashmlp_forward_saved_kernel)) return 1;
    hipLaunchKernelGGL(hashmlp_forward_saved_kernel, dim3((unsigned)cdiv(n, P)), dim3(THREADS), LDS_BYTES, as_stream(stream), *desc, d_positions, d_extra, n,
                       d_out, reinterpret_cast<float*>(d_saved));
    PX_CHECK_HIP(hipGetLastError());
    return 0;
}

int pixie_hashmlp_backward(const pixie_hashmlp_desc* desc, const float* d_positions, const float* d_extra, int64_t n, const float* d_out,
                           const void* d_saved, const float* d_dout, const pixie_hashmlp_grads* grads, void* d_scratch, void* stream) {
    const char* what = "pixie_hashmlp_backward";
    if (check_call(desc, d_positions, d_extra, n, what)) return 1;
    PX_REQUIRE(grads != nullptr, "%s: grads is null", what);
    const pixie_hashmlp_desc& m = *desc;
    const int F = m.n_levels > 0 ? m.features_per_level : 0, n_grid = m.n_levels * F;
    PX_REQUIRE(grads->d_table == nullptr || n_grid > 0, "%s: d_table given for a network without a grid", what);
    PX_REQUIRE(grads->d_extra == nullptr || m.n_extra > 0, "%s: d_extra given for a network without extra columns", what);
    for (int i = m.n_hidden + 1; i < PIXIE_HASHMLP_MAX_LAYERS; ++i)
        PX_REQUIRE(grads->d_weight[i] == nullptr && grads->d_bias[i] == nullptr, "%s: gradient pointer for layer %d of %d", what, i, m.n_hidden + 1);
    hipStream_t st = as_stream(stream);
    bool any = grads->d_table != nullptr || grads->d_extra != nullptr;
    for (int i = 0; i <= m.n_hidden; ++i) any = any || grads->d_weight[i] != nullptr || grads->d_bias[i] != nullptr;
    if (!any) return 0;
    if (n == 0)
        return zero_empty_grads(*grads, m.n_hidden + 1, (size_t)m.table_rows * F, [&m](int i) { return std::make_pair(hmp::layer_out(m, i), hmp::layer_in(m, i)); }, st);
    PX_REQUIRE(d_out != nullptr && d_saved != nullptr && d_dout != nullptr, "%s: d_out, d_saved or d_dout is null", what);
    PX_REQUIRE(d_scratch != nullptr && (reinterpret_cast<uintptr_t>(d_scratch) & 255) == 0, "%s: d_scratch is null or not 256-byte aligned", what);
    const hmp::ScratchLayout L = hmp::scratch_layout(m, n);
    char* base = reinterpret_cast<char*>(d_scratch);
    unsigned int* header = reinterpret_cast<unsigned int*>(base);
    float* dz = reinterpret_cast<float*>(base + L.dz);
    float* dxg = reinterpret_cast<float*>(base + L.dxg);
    float* part = reinterpret_cast<float*>(base + L.part);
    unsigned long long* acc = reinterpret_cast<unsigned long long*>(base + L.acc);
    const float* saved = reinterpret_cast<const float*>(d_saved);
    const int in_dim = hg::input_width(m);

    PX_CHECK_HIP(hipMemsetAsync(header, 0, hmp::kHeaderBytes, st));
    if (grads->d_table != nullptr) PX_CHECK_HIP(hipMemsetAsync(acc, 0, 8 * (size_t)m.table_rows * F, st));
    hipLaunchKernelGGL(hashmlp_backward_kernel, dim3((unsigned)cdiv(n, P)), dim3(THREADS), 0, st, m, n, d_out, d_dout, saved, dz,
                       grads->d_table != nullptr ? dxg : (float*)nullptr, grads->d_extra, header);
    PX_CHECK_HIP(hipGetLastError());

    for (int i = 0; i <= m.n_hidden; ++i) {
        if (grads->d_weight[i] == nullptr && grads->d_bias[i] == nullptr) continue;
        const int O = hmp::layer_out(m, i), K = hmp::layer_in(m, i), k_tiles = (K + 63) / 64, o_tiles = (O + 63) / 64;
        const int slabs = hmp::launched_slabs(n, O, K);
        const int64_t cps = hmp::chunks_per_slab(n, O, K);
        float* bpart = part + (int64_t)slabs * O * K;
        const float* A = i == 0 ? saved : saved + (int64_t)in_dim * n + (int64_t)(i - 1) * 64 * n;
        const dim3 grid((unsigned)(o_tiles * k_tiles), (unsigned)slabs);
        if (i == m.n_hidden)
            hipLaunchKernelGGL(weight_grad_kernel<true>, grid, dim3(THREADS), 0, st, d_dout, d_out, m.out_activation, A, n, O, K, k_tiles, cps, part, bpart);
        else
            hipLaunchKernelGGL(weight_grad_kernel<false>, grid, dim3(THREADS), 0, st, (const float*)(dz + (int64_t)i * 64 * n), (const float*)nullptr, 0, A, n,
                               O, K, k_tiles, cps, part, bpart);
        PX_CHECK_HIP(hipGetLastError());
        hipLaunchKernelGGL(slab_sum_kernel, dim3((unsigned)cdiv(O * K + O, 256)), dim3(256), 0, st, (const float*)part, (const float*)bpart, slabs, O, K,
                           grads->d_weight[i], grads->d_bias[i]);
        PX_CHECK_HIP(hipGetLastError());
    }

    if (grads->d_table != nullptr) return finish_table_grad(table_scatter_kernel, THREADS, m, d_positions, n, dxg, header, acc, grads->d_table, st);
    return 0;
}

}  // extern "C"
