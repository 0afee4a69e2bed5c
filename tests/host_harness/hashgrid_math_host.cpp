// tests/host_harness/hashgrid_math_host.cpp -- compiles pixie_amd/csrc/hashgrid_math.h for the HOST so that CPU-only tests can check
// the arithmetic of the feature-field query before any GPU run: the level tables of both grid conventions, the lattice coordinate,
// affine, contraction / aabb and selector, and per level the cell, the 8 corner rows, their weights and the blended columns, through
// the same header functions in the same order as encode_tile and tile_positions of field_query.hip, as sequential loops.
// With -DHG_STANDALONE it is a program of its own (main below) for -fsanitize=address,undefined: every table it gathers from has
// exactly the rows the level table asks for, so a corner row past the end is a heap overflow the sanitizer reports.
// Test infrastructure only: the product never executes this.
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../pixie_amd/csrc/hashgrid_math.h"

namespace hg = pixie::hg;

extern "C" {

// convention 0 = nerfstudio, 1 = tcnn (per_level_scale from the same growth formula)
int hh_hg_levels(int convention, int n_levels, int base_res, int max_res, int log2_T, hg::Level* out, int64_t* total) {
    if (convention == 0) return hg::levels_nerfstudio(n_levels, base_res, max_res, log2_T, out, total);
    const double growth = n_levels > 1 ? exp((log((double)max_res) - log((double)base_res)) / (n_levels - 1)) : 1.0;
    return hg::levels_tcnn(n_levels, base_res, growth, log2_T, out, total);
}

void hh_hg_lattice(double min_bound, double voxel_size, int n, float* out) {
    for (int i = 0; i < n; ++i) out[i] = hg::lattice_coord(min_bound, voxel_size, i);
}

void hh_hg_unit(const float* A, int contraction, const float* aabb, const float* x, int64_t n, float* p, int32_t* sel) {
    for (int64_t i = 0; i < n; ++i) {
        hg::affine(A, x + 3 * i, p + 3 * i);
        if (contraction) hg::contract_linf(p + 3 * i); else hg::normalise_aabb(aabb, p + 3 * i);
        sel[i] = hg::selector(p + 3 * i);
    }
}

// the same through hg::unit_position, the function the kernels call; A may be null (no affine)
void hh_hg_unit_position(const float* A, int contraction, const float* aabb, const float* x, int64_t n, float* p, int32_t* sel) {
    for (int64_t i = 0; i < n; ++i) sel[i] = hg::unit_position(A, contraction, aabb, x + 3 * i, p + 3 * i);
}

// rows (n, 8) and weights (n, 8) of one level
void hh_hg_corners(const hg::Level* lv, const float* p, int64_t n, uint32_t* rows, float* weights) {
    for (int64_t i = 0; i < n; ++i) {
        const hg::Cell s = hg::cell_of(*lv, p + 3 * i);
        for (int k = 0; k < 8; ++k) {
            rows[8 * i + k] = hg::corner_row_k(*lv, s, k);
            weights[8 * i + k] = hg::corner_weight(s, k);
        }
    }
}

// out (n, L F): the float32 blend in the kernel's order (corner 0..7, f += w * t)
void hh_hg_encode(const hg::Level* lv, int n_levels, const float* table, int F, const float* p, int64_t n, float* out) {
    for (int64_t i = 0; i < n; ++i)
        for (int l = 0; l < n_levels; ++l) {
            const hg::Cell s = hg::cell_of(lv[l], p + 3 * i);
            float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 8; ++k) {
                const float w = hg::corner_weight(s, k);
                const float* row = table + (size_t)hg::corner_row_k(lv[l], s, k) * F;
                for (int c = 0; c < F; ++c) f[c] += w * row[c];
            }
            for (int c = 0; c < F; ++c) out[(i * n_levels + l) * F + c] = f[c];
        }
}

void hh_hg_frequency_args(const float* p, int64_t n, int n_freq, float* out) {
    for (int64_t i = 0; i < n; ++i)
        for (int j = 0; j < 6 * n_freq; ++j) out[i * 6 * n_freq + j] = hg::frequency_arg(p + 3 * i, j, n_freq);
}

}  // extern "C"

#ifdef HG_STANDALONE
int main() {
    const int cfg[3][4] = {{4, 4, 32, 8}, {12, 16, 128, 19}, {16, 16, 2048, 19}};
    uint32_t state = 12345u;
    auto rnd = [&]() { state = state * 1664525u + 1013904223u; return (float)(state >> 8) / 16777216.0f; };
    double sum = 0;
    for (int conv = 0; conv < 2; ++conv)
        for (const auto& c : cfg) {
            hg::Level lv[hg::kMaxLevels];
            int64_t total = 0;
            if (hh_hg_levels(conv, c[0], c[1], c[2], c[3], lv, &total)) return 1;
            const int F = 2;
            std::vector<float> table((size_t)total * F);
            for (auto& t : table) t = rnd() - 0.5f;
            const int n = 4096;
            std::vector<float> p(3 * n), out((size_t)n * c[0] * F);
            for (auto& v : p) v = rnd();
            const float edge[6] = {0.f, 1.f, 0.5f, 0.25f, 1.f, 0.f};             // exactly 0, exactly 1, cell boundaries
            for (int i = 0; i < 6; ++i) p[i] = edge[i], p[6 + i] = edge[5 - i];
            hh_hg_encode(lv, c[0], table.data(), F, p.data(), n, out.data());
            for (float v : out) sum += v;
            printf("convention %d levels %d base %d max %d log2_T %d: %lld rows\n", conv, c[0], c[1], c[2], c[3], (long long)total);
        }
    const float A[12] = {0.9f, 0.1f, 0.f, 0.05f, -0.1f, 0.9f, 0.f, 0.f, 0.f, 0.f, 1.1f, -0.02f}, aabb[6] = {-1, -1, -1, 1, 1, 1};
    std::vector<float> x(3 * 512), q(3 * 512);
    std::vector<int32_t> sel(512);
    for (auto& v : x) v = 6.f * rnd() - 3.f;
    hh_hg_unit(A, 1, aabb, x.data(), 512, q.data(), sel.data());
    hh_hg_unit(A, 0, aabb, x.data(), 512, q.data(), sel.data());
    for (int contraction = 0; contraction < 2; ++contraction) {
        hh_hg_unit_position(A, contraction, aabb, x.data(), 512, q.data(), sel.data());
        hh_hg_unit_position(nullptr, contraction, aabb, x.data(), 512, q.data(), sel.data());
    }
    printf("checksum %.6f\nok\n", sum);
    return 0;
}
#endif
