// map_field.hpp -- the distance field of a map region, an exact Euclidean distance transform truncated at a radius, and the cell
// range of a box on the host (map_field.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_distance_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                        int32_t radius_cells, int32_t *d_dist2, float *launch_ms, hipStream_t stream,  // launch_ms[4] or NULL
                        long long *outer_bracket = nullptr);  // not NULL: the stage bracket is opened into it and left to the caller
int box_to_cells(int depth, const float center[3], float edge, const float box[6], int32_t lo[3], int32_t hi[3], int32_t *empty);
}  // namespace svoslam
