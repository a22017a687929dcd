// map_score.hpp -- scoring candidate poses against a distance field of a map region: every sensor point moved by every pose, its
// cell looked up in the field, the values summed per pose, and the best pose (map_score.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int score_poses(svoslam_workspace *ws, const int32_t *d_dist2, int depth, const float center[3], float edge, const int32_t origin[3],
                const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, int32_t n_poses, int32_t miss_cost,
                int32_t min_near, int64_t *d_cost, int32_t *d_near, int32_t *d_far, int32_t *d_outside, int64_t *d_best,
                hipStream_t stream);  // every output may be NULL, with n_poses > 0 not all
}  // namespace svoslam
