// pixie_amd/csrc/raster_batch_plan.h -- how pixie_raster_forward_batch partitions the views of a batch into sort groups.
//
// A pure host function, no HIP: raster.hip calls it between the one read-back of the per-view instance counts and the per-group
// launches, and tests/test_raster_batch_plan.py builds it alone with g++ and compares it with a Python restatement.
// Greedy over consecutive views: a group takes views while its instance total stays within `capacity` (what one sort's buffers
// hold) and its view count within `max_views` (so that view * tiles + tile fits the upper 32 key bits).  Views with no instance
// cost nothing and join the group they fall into.
#pragma once
#include <stdint.h>

namespace pixie {
namespace raster {

// Writes the group boundaries to begin[0 .. groups] (begin[0] = 0, begin[groups] = views; room for views + 1 entries) and returns
// the number of groups (views >= 1).  If view v alone holds more than `capacity` instances nothing can render it: returns
// -1 - v for the first such view.  max_views >= 1.
inline int64_t plan_groups(const uint64_t* counts, int views, uint64_t capacity, int max_views, int32_t* begin) {
    for (int v = 0; v < views; ++v)
        if (counts[v] > capacity) return -1 - (int64_t)v;
    int64_t groups = 0;
    int v = 0;
    while (v < views) {
        begin[groups++] = v;
        uint64_t total = 0;
        int taken = 0;
        while (v < views && taken < max_views && counts[v] <= capacity - total) {
            total += counts[v];
            ++taken;
            ++v;
        }
    }
    begin[groups] = views;
    return groups;
}

}  // namespace raster
}  // namespace pixie
