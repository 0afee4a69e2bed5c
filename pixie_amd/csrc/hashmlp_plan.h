// pixie_amd/csrc/hashmlp_plan.h -- the host policy of the 64-wide hash-grid MLP's training pass (field_query_backward.hip): layer shapes,
// the slabs of the weight gradient and the byte layout of the saved activations and the scratch, as pure functions, so that
// tests/test_hashmlp_plan_host.py can build them with g++ alone and hold them to the formula of include/pixie_hip.h.  Every function
// is a template over the descriptor (pixie_hashmlp_desc: n_levels, features_per_level, n_frequencies, n_extra, n_hidden, out_dim,
// table_rows), so that this header needs no pixie_hip.h.  The width of the encoded input row is hashgrid_math.h's input_width.
//
//   slabs    the weight gradient of an (out, in) layer is summed over fixed slabs of points, one workgroup per (64 x 64 block, slab).
//            slab_count is what the scratch is sized for; launched_slabs is what is launched: whole tiles of 64 points per slab, so fewer slabs
//            may be needed than were asked for, never more.  Both are pure functions of n and the shape.
//   scratch  header | dZ of the hidden layers [n_hidden][64][n] | dX of the grid columns [levels * F][n] | slab partials of the largest
//            layer | 64-bit accumulators of the table gradient; every region 256-byte aligned
#pragma once
#include <stdint.h>

#include "hashgrid_math.h"

namespace pixie {
namespace hmp {

// points per workgroup of the tile kernels; hidden units; bytes of the scratch header; the slab policy's two limits
constexpr int kTile = 64, kWidth = 64, kHeaderBytes = 256, kMaxSlabs = 256, kTargetBlocks = 1024;

template <class D> inline int layer_out(const D& m, int i) { return i == m.n_hidden ? m.out_dim : kWidth; }
template <class D> inline int layer_in(const D& m, int i) { return i == 0 ? hg::input_width(m) : kWidth; }

inline int64_t round256(int64_t b) { return (b + 255) / 256 * 256; }
inline int64_t tiles_of(int64_t n) { return n > 0 ? (n + kTile - 1) / kTile : 1; }      // n = 0 is planned as one empty tile

// how many slabs of points the weight gradient of an (out, in) layer is cut into at most
inline int slab_count(int64_t n, int out, int in) {
    int64_t s = kTargetBlocks / ((int64_t)((out + 63) / 64) * ((in + 63) / 64));
    if (s > kMaxSlabs) s = kMaxSlabs;
    if (s > tiles_of(n)) s = tiles_of(n);
    return s < 1 ? 1 : (int)s;
}

// tiles per slab, and the slabs that then own a tile: 1 <= launched_slabs <= slab_count, chunks_per_slab * launched_slabs >= tiles
inline int64_t chunks_per_slab(int64_t n, int out, int in) { return (tiles_of(n) + slab_count(n, out, in) - 1) / slab_count(n, out, in); }
inline int launched_slabs(int64_t n, int out, int in) { return (int)((tiles_of(n) + chunks_per_slab(n, out, in) - 1) / chunks_per_slab(n, out, in)); }

template <class D> inline int64_t saved_bytes(const D& m, int64_t n) { return 4 * n * ((int64_t)hg::input_width(m) + kWidth * m.n_hidden); }

struct ScratchLayout { int64_t dz, dxg, part, acc, total; };      // byte offsets; the header is at 0

template <class D> inline ScratchLayout scratch_layout(const D& m, int64_t n) {
    ScratchLayout L;
    const int F = m.n_levels > 0 ? m.features_per_level : 0;
    L.dz = kHeaderBytes;
    L.dxg = L.dz + round256(4 * (int64_t)kWidth * m.n_hidden * n);
    L.part = L.dxg + round256(4 * (int64_t)m.n_levels * F * n);
    int64_t floats = 0;
    for (int i = 0; i <= m.n_hidden; ++i) {
        const int64_t o = layer_out(m, i), k = layer_in(m, i), f = (int64_t)slab_count(n, (int)o, (int)k) * (o * k + o);
        if (f > floats) floats = f;
    }
    L.acc = L.part + round256(4 * floats);
    L.total = L.acc + round256(8 * m.table_rows * F);
    return L;
}

}  // namespace hmp
}  // namespace pixie
