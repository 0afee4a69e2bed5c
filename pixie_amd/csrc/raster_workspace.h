// pixie_amd/csrc/raster_workspace.h -- how pixie_raster_forward lays its workspace out, shared with the backward pass
// (raster_backward.hip), which reads what the forward left there: centre, conic_opacity, offsets, ranges and the sorted instance list.
#pragma once
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <cstddef>
#include <cstdint>

#include "common.h"

namespace pixie {
namespace raster_ws {

// Workspace: the part steps 1-2 need, whose size depends on (n, tiles) only, then the part sized by the instance count.
struct Layout {
    size_t depth, centre, conic_opacity, tiles_touched, offsets, ranges, scan_temp, scan_temp_bytes, fixed_bytes;
    size_t keys_in, keys_out, vals_in, vals_out, sort_temp, sort_temp_bytes, total_bytes;
};

inline size_t take(size_t& cursor, size_t bytes) {
    const size_t at = cursor;
    cursor = (cursor + bytes + 255) & ~(size_t)255;
    return at;
}

inline int sort_end_bit(int tiles) {
    int bits = 0;
    while ((1LL << bits) < tiles) ++bits;
    return 32 + bits;
}

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
    const size_t m = (size_t)instances;
    L.keys_in = take(cur, sizeof(uint64_t) * m);
    L.keys_out = take(cur, sizeof(uint64_t) * m);
    L.vals_in = take(cur, sizeof(uint32_t) * m);
    L.vals_out = take(cur, sizeof(uint32_t) * m);
    L.sort_temp_bytes = 0;
    if (m > 0)
        PX_CHECK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, L.sort_temp_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                                        (const uint32_t*)nullptr, (uint32_t*)nullptr, m, 0, sort_end_bit(tiles)));
    L.sort_temp = take(cur, L.sort_temp_bytes);
    L.total_bytes = cur;
    return 0;
}

}  // namespace raster_ws
}  // namespace pixie
