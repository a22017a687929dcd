// map_plan.hpp -- path planning in a map region: the weighted cost-to-go field and the paths traced down a field (map_plan.hip; own
// specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_cost_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                    int32_t clearance_cells, int32_t comfort_cells, const int32_t *h_ring_cost, const int32_t *d_seeds, int32_t n_seeds,
                    int32_t *d_cost, svoslam_plan_stats *stats, hipStream_t stream);
int field_trace_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], const int32_t *d_starts, int32_t n_starts,
                      int32_t max_cells, int32_t *d_paths, int32_t *d_lengths, hipStream_t stream);
}  // namespace svoslam
