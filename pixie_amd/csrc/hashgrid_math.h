// pixie_amd/csrc/hashgrid_math.h -- the arithmetic of the NeRF feature-field query (field_query.hip) that decides cells, corners
// and the selector, as __host__ __device__ functions, so that tests/host_harness/hashgrid_math_host.cpp can run the same lines
// on the CPU (g++ -ffp-contract=off) against the NumPy restatement of tests/_field_query_ref.py.
//
// Everything up to the scaled position q of a level is float32, unfused, in the order written here:
//   lattice      x_i = float32(double(min) + i * double(voxel_size)), unless the caller supplies the axes (torch.arange on the CPU
//                fills its vector lanes in float32 and lands up to a few ulps away, depending on the vector width)
//   affine       n_r = ((A[r][0] x + A[r][1] y) + A[r][2] z) + A[r][3]
//   contraction  m = max(|x|, |y|, |z|);  m < 1 ? p : (2 - 1 / m) * (p / m);  then (p + 2) / 4
//   aabb         (p - lo) / (hi - lo)
//   selector     all of 0 < p < 1; the density net sees p * selector
//   level        q = p * scale + shift;  c0 = floor(q);  w = q - c0
// A level is {scale, shift, res, size, offset, dense}: corner (x, y, z) of the cell has the table row
//   (dense ? x + y res + z res^2 : x ^ y 2654435761 ^ z 805459861)  [uint32]  % size + offset
// which serves both nerfstudio's torch hash encoding (scale = floor(min_res g^l) in float32, shift 0, always hashed, size 2^T, offset l 2^T)
// and tiny-cuda-nn's grid (scale = 2^(l log2 s) base - 1, shift 0.5, res = ceil(scale) + 1, dense while res^3 <= 2^T, levels
// packed one after another, each rounded up to 8 rows).
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define HG_HD __host__ __device__ inline
#else
#define HG_HD inline
#endif

namespace pixie {
namespace hg {

struct Level {
    float scale, shift;
    uint32_t res, size, offset, dense;
};

// a descriptor's level (pixie_hashgrid_level: the same six fields) as a Level; a template so that this header needs no pixie_hip.h
template <class L> HG_HD Level level_of(const L& v) { return Level{v.scale, v.shift, v.res, v.size, v.offset, v.dense}; }

constexpr int kMaxLevels = 16;
constexpr uint32_t kPrimeY = 2654435761u, kPrimeZ = 805459861u;

// ---- host-side level tables -----------------------------------------------------------------------------------------------
// nerfstudio: growth = exp((ln max_res - ln min_res) / (L - 1)) in double, scale = floor(min_res growth^l) in FLOAT32: the module
// raises the double to an integer tensor, which torch evaluates in its default dtype, so (16, 2048, 16 levels) ends at 2047, not 2048
inline int levels_nerfstudio(int n_levels, int min_res, int max_res, int log2_T, Level* out, int64_t* total) {
    if (n_levels < 1 || n_levels > kMaxLevels || min_res < 1 || max_res < min_res || log2_T < 1 || log2_T > 24) return 1;
    const double growth = n_levels > 1 ? exp((log((double)max_res) - log((double)min_res)) / (n_levels - 1)) : 1.0;
    const uint32_t T = 1u << log2_T;
    for (int l = 0; l < n_levels; ++l) {
        Level& v = out[l];
        v.scale = floorf((float)min_res * powf((float)growth, (float)l));
        v.shift = 0.0f;
        v.res = (uint32_t)v.scale + 1u;
        v.size = T;
        v.offset = (uint32_t)l * T;
        v.dense = 0;
    }
    *total = (int64_t)n_levels * T;
    return 0;
}

// tiny-cuda-nn: per_level_scale s is given (the caller's growth factor), scale = exp2(l log2 s) base - 1, evaluated in double and
// rounded once (the library evaluates it in float32 on the device, which may differ in the last place of the scale)
inline int levels_tcnn(int n_levels, int base_res, double per_level_scale, int log2_T, Level* out, int64_t* total) {
    if (n_levels < 1 || n_levels > kMaxLevels || base_res < 1 || !(per_level_scale >= 1.0) || log2_T < 1 || log2_T > 24) return 1;
    const uint32_t T = 1u << log2_T;
    const double log2s = log2(per_level_scale);
    uint64_t offset = 0;
    for (int l = 0; l < n_levels; ++l) {
        Level& v = out[l];
        v.scale = (float)(exp2((double)l * log2s) * (double)base_res - 1.0);
        v.shift = 0.5f;
        v.res = (uint32_t)ceilf(v.scale) + 1u;
        const uint64_t cube = (uint64_t)v.res * v.res * v.res;
        v.dense = cube <= T ? 1u : 0u;
        const uint64_t padded = (cube + 7u) / 8u * 8u;
        v.size = (uint32_t)(padded < T ? padded : T);
        v.offset = (uint32_t)offset;
        offset += v.size;
        if (offset > 0xffffffffull) return 1;
    }
    *total = (int64_t)offset;
    return 0;
}

// ---- per point ------------------------------------------------------------------------------------------------------------
HG_HD float lattice_coord(double min_bound, double voxel_size, int i) { return (float)(min_bound + (double)i * voxel_size); }

HG_HD void affine(const float* A, const float* x, float* out) {              // A: 3 x 4 row-major
    for (int r = 0; r < 3; ++r) {
        float t = A[4 * r + 0] * x[0];
        t = t + A[4 * r + 1] * x[1];
        t = t + A[4 * r + 2] * x[2];
        out[r] = t + A[4 * r + 3];
    }
}

HG_HD void contract_linf(float* p) {                                         // in place, then (p + 2) / 4
    const float m = fmaxf(fabsf(p[0]), fmaxf(fabsf(p[1]), fabsf(p[2])));
    if (!(m < 1.0f)) {
        const float f = 2.0f - 1.0f / m;
        for (int a = 0; a < 3; ++a) p[a] = f * (p[a] / m);
    }
    for (int a = 0; a < 3; ++a) p[a] = (p[a] + 2.0f) / 4.0f;
}

HG_HD void normalise_aabb(const float* aabb, float* p) {                     // aabb: lo[3], hi[3]
    for (int a = 0; a < 3; ++a) p[a] = (p[a] - aabb[a]) / (aabb[3 + a] - aabb[a]);
}

HG_HD int selector(const float* p) {
    return (p[0] > 0.0f && p[0] < 1.0f && p[1] > 0.0f && p[1] < 1.0f && p[2] > 0.0f && p[2] < 1.0f) ? 1 : 0;
}

// x -> unit-cube position q (distinct from x): the affine if A is given, then the contraction or the aabb.  Returns the selector;
// what it masks is the caller's business.
HG_HD int unit_position(const float* A, int contraction, const float* aabb, const float* x, float* q) {
    if (A != nullptr) affine(A, x, q);
    else { q[0] = x[0]; q[1] = x[1]; q[2] = x[2]; }
    if (contraction) contract_linf(q); else normalise_aabb(aabb, q);
    return selector(q);
}

struct Cell {
    uint32_t c[3];     // floor(q), as the uint32 the corner index is formed in (negative cells wrap)
    float w[3];        // q - floor(q)
};

HG_HD Cell cell_of(const Level& lv, const float* p) {
    Cell s;
    for (int a = 0; a < 3; ++a) {
        float q = p[a] * lv.scale;
        q = q + lv.shift;
        const float f = floorf(q);
        s.w[a] = q - f;
        s.c[a] = (uint32_t)(int32_t)f;
    }
    return s;
}

HG_HD uint32_t corner_row(const Level& lv, uint32_t x, uint32_t y, uint32_t z) {
    const uint32_t i = lv.dense ? x + y * lv.res + z * lv.res * lv.res : (x ^ (y * kPrimeY) ^ (z * kPrimeZ));
    return i % lv.size + lv.offset;
}

// corner k in 0..7: bit 0 = x + 1, bit 1 = y + 1, bit 2 = z + 1
HG_HD uint32_t corner_row_k(const Level& lv, const Cell& s, int k) {
    return corner_row(lv, s.c[0] + (uint32_t)(k & 1), s.c[1] + (uint32_t)((k >> 1) & 1), s.c[2] + (uint32_t)((k >> 2) & 1));
}

HG_HD float corner_weight(const Cell& s, int k) {
    const float wx = (k & 1) ? s.w[0] : 1.0f - s.w[0];
    const float wy = (k & 2) ? s.w[1] : 1.0f - s.w[1];
    const float wz = (k & 4) ? s.w[2] : 1.0f - s.w[2];
    return wx * wy * wz;
}

// columns of the encoded row of a network descriptor: the grid's, the frequency block's, then the extra input columns
template <class D> HG_HD int input_width(const D& m) { return m.n_levels * m.features_per_level + 6 * m.n_frequencies + m.n_extra; }

// Frequency block, tiny-cuda-nn's ordering: output j of 3 * 2 * n has dim j / (2 n), octave (j / 2) % n, phase (j % 2) pi / 2,
// value sin(2^octave pi x + phase); the odd outputs are taken as the cosine of the same argument.
HG_HD float frequency_arg(const float* p, int j, int n_freq) {
    const int dim = j / (2 * n_freq), octave = (j / 2) % n_freq;
    return (p[dim] * (float)(1u << octave)) * 3.14159265358979323846f;
}

}  // namespace hg
}  // namespace pixie
