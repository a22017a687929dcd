// map_reach.hpp -- the reach field of a map region: shortest free-path steps from seed cells (map_reach.hip; own specification,
// DESIGN.md section 16)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_reach_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t clearance_cells, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_steps, svoslam_reach_stats *stats,
                     hipStream_t stream);
}  // namespace svoslam
