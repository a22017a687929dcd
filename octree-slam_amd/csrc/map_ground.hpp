// map_ground.hpp -- ground navigation in a map region (map_ground.hip): the foothold cost field and the paths
// traced down it
#pragma once
#include "workspace.hpp"

namespace svoslam {

int pool_ground_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                      int32_t up, int32_t r, int32_t H, int32_t S, int32_t c, int32_t snap, const int32_t *d_seeds, int32_t n_seeds,
                      int32_t *d_cost, svoslam_ground_stats *stats, hipStream_t stream);
int field_trace_ground_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], int32_t up, int32_t S, int32_t c,
                             int32_t snap, const int32_t *d_starts, int32_t n_starts, int32_t max_cells, int32_t *d_paths,
                             int32_t *d_lengths, hipStream_t stream);

}  // namespace svoslam
