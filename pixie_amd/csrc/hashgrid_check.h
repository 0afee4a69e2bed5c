// pixie_amd/csrc/hashgrid_check.h -- the host check of a descriptor's hash table and level table, shared by every boundary that takes
// one: the 64-wide networks (field_query_body.h) and the proposal density field (density_field.hip).  It has a header of its own, apart
// from hashgrid_table_grad.h, because field_query.hip needs the check and must not receive the training kernels.
#pragma once
#include <cmath>
#include <cstdint>

#include "common.h"

namespace {

// Desc: n_levels, d_table, table_rows, level[]
template <class Desc> int check_grid_table(const Desc& m, const char* what) {
    PX_REQUIRE(m.d_table != nullptr && (reinterpret_cast<uintptr_t>(m.d_table) & 15) == 0, "%s: d_table is null or not 16-byte aligned", what);
    for (int l = 0; l < m.n_levels; ++l) {
        const auto& lv = m.level[l];
        PX_REQUIRE(lv.size > 0 && (int64_t)lv.offset + (int64_t)lv.size <= m.table_rows,
                   "%s: level %d (offset %u, size %u) does not fit the table of %lld rows", what, l, lv.offset, lv.size, (long long)m.table_rows);
        PX_REQUIRE(std::isfinite(lv.scale) && std::isfinite(lv.shift), "%s: level %d has a non-finite scale or shift", what, l);
    }
    return 0;
}

}  // namespace
