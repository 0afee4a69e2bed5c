// pixie_amd/csrc/raster_workspace.h -- the host side that pixie_raster_forward, its batch form (raster.hip) and the backward pass
// (raster_backward.hip) share: the argument checks of a forward descriptor, the width of a sort key, and how the forward lays its
// workspace out, which the backward reads as the forward left it: centre, conic_opacity, offsets, ranges and the sorted instance list.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstddef>
#include <cstdint>

#include "../../include/pixie_hip.h"
#include "common.h"

namespace pixie {
namespace raster_ws {

inline int check_shape(const char* who, int n, int width, int height) {
    PX_REQUIRE(n >= 0, "%s: n %d < 0", who, n);
    PX_REQUIRE(n < INT_MAX, "%s: n %d exceeds one scan (n + 1 counts)", who, n);
    PX_REQUIRE(width > 0 && height > 0, "%s: image %d x %d must be positive", who, width, height);
    PX_REQUIRE(width <= 65536 && height <= 65536, "%s: image %d x %d exceeds 65536 per side", who, width, height);
    return 0;
}

// what a forward needs of its descriptor `f`, whose fields the messages of `who` call `pre`<field>
inline int check_forward_desc(const char* who, const char* pre, const pixie_raster_desc& f) {
    if (check_shape(who, f.n, f.width, f.height)) return 1;
    PX_REQUIRE(f.tanfovx > 0.0f && f.tanfovy > 0.0f, "%s: %stanfovx %g, %stanfovy %g must be positive", who, pre, f.tanfovx, pre, f.tanfovy);
    PX_REQUIRE(f.d_out_color, "%s: null pointer (%sd_out_color is required)", who, pre);
    if (f.n > 0) {
        PX_REQUIRE(f.d_means && f.d_colors && f.d_opacity && f.d_radii, "%s: null pointer (%sd_means, d_colors, d_opacity and d_radii are required)",
                   who, pre);
        PX_REQUIRE((f.d_cov3d != nullptr) != (f.d_scales != nullptr || f.d_rotations != nullptr),
                   "%s: give either %sd_cov3d or the pair d_scales, d_rotations", who, pre);
        PX_REQUIRE(f.d_cov3d || (f.d_scales && f.d_rotations), "%s: %sd_scales and d_rotations go together", who, pre);
    }
    return 0;
}

inline size_t take(size_t& cursor, size_t bytes) {
    const size_t at = cursor;
    cursor = (cursor + bytes + 255) & ~(size_t)255;
    return at;
}

// bits of a sort key: the depth's 32 below the tile index (in a batch: view in group * tiles + tile)
inline int key_bits(int64_t tiles) {
    int bits = 0;
    while ((1LL << bits) < tiles) ++bits;
    return 32 + bits;
}

// the sort's temporary storage for `m` instances over `tiles` tiles
inline int sort_temp_bytes(size_t m, int64_t tiles, size_t& bytes) {
    bytes = 0;
    if (m > 0)
        PX_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, (const uint32_t*)nullptr,
                                                        (uint32_t*)nullptr, m, 0, key_bits(tiles)));
    return 0;
}

// the part of a workspace sized by the instance count: the sort's input and output pairs and its temporary storage
struct SortLayout {
    size_t keys_in, keys_out, vals_in, vals_out, sort_temp;
};

inline void take_sort(size_t& cur, size_t m, size_t temp_bytes, SortLayout& S) {
    S.keys_in = take(cur, sizeof(uint64_t) * m);
    S.keys_out = take(cur, sizeof(uint64_t) * m);
    S.vals_in = take(cur, sizeof(uint32_t) * m);
    S.vals_out = take(cur, sizeof(uint32_t) * m);
    S.sort_temp = take(cur, temp_bytes);
}

// Workspace of a single view: the part the projection and the scan need, whose size depends on (n, tiles) only, then the sort's.
struct Layout : SortLayout {
    size_t depth, centre, conic_opacity, tiles_touched, offsets, ranges, scan_temp, scan_temp_bytes, fixed_bytes, total_bytes;
};

inline int make_layout(int n, int tiles, int64_t instances, Layout& L) {
    size_t cur = 0;
    L.depth = take(cur, sizeof(float) * (size_t)n);
    L.centre = take(cur, sizeof(float2) * (size_t)n);
    L.conic_opacity = take(cur, sizeof(float4) * (size_t)n);
    L.tiles_touched = take(cur, sizeof(uint64_t) * ((size_t)n + 1));
    L.offsets = take(cur, sizeof(uint64_t) * ((size_t)n + 1));
    L.ranges = take(cur, sizeof(uint2) * (size_t)tiles);
    L.scan_temp_bytes = 0;
    PX_CHECK_HIP(hipcub::DeviceScan::ExclusiveSum(nullptr, L.scan_temp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr, n + 1));
    L.scan_temp = take(cur, L.scan_temp_bytes);
    L.fixed_bytes = cur;
    size_t temp = 0;
    if (sort_temp_bytes((size_t)instances, tiles, temp)) return 1;
    take_sort(cur, (size_t)instances, temp, L);
    L.total_bytes = cur;
    return 0;
}

}  // namespace raster_ws
}  // namespace pixie
