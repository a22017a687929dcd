// map_owner.hpp -- the owner field of a map region: the reach field's steps and, with them, which seed is nearest by path
// (map_owner.hip; own specification)
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_owner_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t clearance_cells, const int32_t *d_seeds, int32_t n_seeds, const int32_t *d_seed_field, int32_t *d_steps,
                     int32_t *d_owner, svoslam_owner_stats *stats, hipStream_t stream);
}  // namespace svoslam
