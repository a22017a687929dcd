// map_observe.hpp -- the observed space of a map region: the cells a set of sensor rays passed through and ended in, marked by the
// scatter form of the exact integer supercover walk, and that observation held against the map as six states per cell with the
// frontier between the free and the unknown (map_observe.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
// d_obs: one byte per region cell; d_summary: 6 x int64 (void, outside, far, marked, cells_through, cells_end), may be NULL
int field_observe_rays(svoslam_workspace *ws, uint8_t *d_obs, int depth, const float center[3], float edge, const int32_t origin[3],
                       const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, int32_t n_frames, int32_t range_cells,
                       int32_t accumulate, int64_t *d_summary, hipStream_t stream);
// d_state, d_frontier: one byte per region cell; d_summary: 6 x int32, the cells per state; each may be NULL, not all three
int pool_frontier_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                        const uint8_t *d_obs, uint8_t *d_state, uint8_t *d_frontier, int32_t *d_summary, hipStream_t stream);
}  // namespace svoslam
