// map_nearest.hpp -- the nearest-cell field of a map region: the distance field's value and the witness cell behind it, to the
// occupied or to the free cells (map_nearest.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_nearest_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                       int32_t radius_cells, int32_t which, int32_t *d_dist2, uint64_t *d_cell, int32_t *d_node, uint32_t *d_color,
                       hipStream_t stream);  // every output may be NULL, not all of them
}  // namespace svoslam
