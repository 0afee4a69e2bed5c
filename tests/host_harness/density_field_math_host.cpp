// Host build of pixie_amd/csrc/density_field_math.h (and the hashgrid_math.h front end it sits on) for tests/test_density_field_math.py:
//   g++ -O2 -std=c++17 -ffp-contract=off -fPIC -shared density_field_math_host.cpp
// hh_df_forward walks the kernel's lines for one point after another: front end, per level the 8 corner rows blended in corner
// order, the fmaf chains, in the order density_field.hip runs them.
#include "../../pixie_amd/csrc/density_field_math.h"
#include "../../pixie_amd/csrc/hashgrid_math.h"

using namespace pixie;

extern "C" {

// x (3) -> masked unit position p (3); returns the selector.  A: 12 floats or null; aabb: 6 floats
int hh_df_front(const float* x, const float* A, int contraction, const float* aabb, float* p, float* unmasked) {
    if (A != nullptr) hg::affine(A, x, p);
    else for (int a = 0; a < 3; ++a) p[a] = x[a];
    if (contraction) hg::contract_linf(p);
    else hg::normalise_aabb(aabb, p);
    for (int a = 0; a < 3; ++a) unmasked[a] = p[a];
    const int sel = hg::selector(p);
    if (!sel) p[0] = p[1] = p[2] = 0.0f;
    return sel;
}

float hh_df_network(int n_hidden, int in_dim, const float* w0, const float* w1, const float* w2, const float* b0, const float* b1,
                    const float* b2, const float* x, float* zs) {
    const float* w[3] = {w0, w1, w2};
    const float* b[3] = {b0, b1, b2};
    return df::network(n_hidden, in_dim, w, b, x, zs);
}

// positions (n, 3) -> h (n), p (n, 3) unmasked unit positions, sel (n)
void hh_df_forward(const hg::Level* levels, int n_levels, int F, const float* table, int n_hidden, const float* w0, const float* w1,
                   const float* w2, const float* b0, const float* b1, const float* b2, const float* A, int contraction, const float* aabb,
                   const float* positions, int64_t n, float* h, float* p_out, int* sel_out) {
    const float* w[3] = {w0, w1, w2};
    const float* b[3] = {b0, b1, b2};
    for (int64_t i = 0; i < n; ++i) {
        float p[3];
        sel_out[i] = hh_df_front(positions + 3 * i, A, contraction, aabb, p, p_out + 3 * i);
        float x[df::kMaxInput];
        for (int l = 0; l < n_levels; ++l) {
            const hg::Cell c = hg::cell_of(levels[l], p);
            float f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (int k = 0; k < 8; ++k) {
                const float wk = hg::corner_weight(c, k);
                const float* row = table + (size_t)hg::corner_row_k(levels[l], c, k) * F;
                for (int q = 0; q < F; ++q) f[q] += wk * row[q];
            }
            for (int q = 0; q < F; ++q) x[l * F + q] = f[q];
        }
        h[i] = df::network(n_hidden, n_levels * F, w, b, x, nullptr);
    }
}

float hh_df_density(float h, float aid) { return df::density_of(h, aid); }
float hh_df_dh(float g, float h, float aid, int sel) { return df::dh_of(g, h, aid, sel); }
int hh_df_forward_blocks(int64_t n) { return df::forward_blocks(n); }
int hh_df_slab_count(int64_t n) { return df::slab_count(n); }
int hh_df_param_count(int in_dim, int n_hidden) { return df::param_count(in_dim, n_hidden); }
int hh_df_weight_offset(int in_dim, int n_hidden, int i) { return df::weight_offset(in_dim, n_hidden, i); }
int64_t hh_df_saved_bytes(int64_t n) { return df::saved_bytes(n); }
void hh_df_scratch(int64_t n, int in_dim, int n_hidden, int64_t rows, int F, int64_t* out) {
    const df::Scratch L = df::scratch_layout(n, in_dim, n_hidden, rows, F);
    out[0] = L.pos; out[1] = L.dxg; out[2] = L.part; out[3] = L.acc; out[4] = L.total;
}

}  // extern "C"
