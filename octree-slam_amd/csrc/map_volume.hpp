// map_volume.hpp -- asking the map by volume: occupied cells in a box and the nearest occupied cell to a point (map_volume.hip; own
// specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_count_boxes(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_boxes, int64_t stop_after,
                     int32_t n, uint64_t *d_count, uint64_t *d_first_cell, int32_t *d_first_node, uint32_t *d_steps, hipStream_t stream);
int pool_nearest_occupied(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_points,
                          int32_t radius_cells, int32_t n, int32_t *d_dist2, uint64_t *d_cell, int32_t *d_node, uint32_t *d_color,
                          uint32_t *d_steps, hipStream_t stream);
}  // namespace svoslam
