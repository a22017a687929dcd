// map_coverage.hpp -- viewpoints that cover a map region: the candidates' sight of a compacted list of target cells as a bit matrix,
// and a greedy set cover over it (map_coverage.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_cover_views(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t range_cells, int32_t target_mode, const uint8_t *d_select, const int32_t *d_cands, int32_t n_cands,
                     int32_t k_max, int32_t min_gain, int32_t *d_seen, int32_t *d_chosen, int32_t *d_gain, int32_t *d_round,
                     int32_t *d_summary, hipStream_t stream);  // d_select, d_seen and d_round may be NULL
}  // namespace svoslam
