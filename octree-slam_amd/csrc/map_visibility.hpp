// map_visibility.hpp -- the visibility field of a map region: for every cell of a box of cells the viewpoints with a free line of
// sight to it within a range, by an exact integer supercover walk (map_visibility.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_visibility_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                          int32_t range_cells, const int32_t *d_views, int32_t n_views, uint32_t *d_mask, int32_t *d_count,
                          hipStream_t stream);  // either output may be NULL, not both
}  // namespace svoslam
