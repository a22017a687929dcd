// map_components.hpp -- the component labels of a map region: connected free or solid cells (map_components.hip; own
// specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_label_components(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                          int32_t clearance_cells, int32_t which, int32_t *d_labels, int32_t *d_sizes,
                          svoslam_component_stats *stats, hipStream_t stream);
}  // namespace svoslam
