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
#include "field_query_body.h"

namespace {

__global__ __launch_bounds__(THREADS) void hashmlp_forward_kernel(const pixie_hashmlp_desc m, const float* d_positions, const float* d_extra,
                                                                  int64_t n, float* d_out) {
    extern __shared__ float lds[];
    float *X = lds + X_OFF, *H = lds + H_OFF, *wl = lds + WL_OFF, *pos = lds + POS_OFF;
    const int64_t tile0 = (int64_t)blockIdx.x * P;
    load_tile_positions(d_positions, tile0, n, pos);
    encode_tile(m, pos, d_extra, tile0, n, X);
    const float* hid = hidden_layers(m, hg::input_width(m), X, X, H, wl);
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
            // hg::unit_position, written out: through the call the compiler schedules these kernels differently (same registers), and
            // scripts/device_code_identity.py against the parent is the bar for this family's helpers
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
    const float* hid = hidden_layers(v.density, hg::input_width(v.density), X, X, H, wl);
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
    const float* hid = hidden_layers(v.feature, hg::input_width(v.feature), X, X, H, wl);
    output_layer<HALF>(v.feature, hid, X, wl, aux, d_features, tile0, n);
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
