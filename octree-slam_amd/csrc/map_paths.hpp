// map_paths.hpp -- the clearance of segments over a distance field, and planned paths straightened by line of sight without giving
// up their clearance (map_paths.hip; own specification).  The walk both use is supercover_walk.hpp.
//
// d_dist2 is a field as svoslam_pool_distance_field writes it.  field_shorten_paths cannot check the field's radius: the caller must
// supply one computed with a radius >= clearance_cells, or cells nearer than that pass for clear.  A region has at most 2^16 cells
// per axis (the bound of the walk's int64 keys) and 2^31 - 1 in all.  With max_lookahead = 0 a path of L cells costs O(L^2) walks in
// the worst case; max_lookahead = W bounds it by L * W.
#pragma once
#include "common.hpp"

namespace svoslam {
int field_segment_clearance(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], const int32_t *d_segments, int32_t n,
                            int32_t *d_min, int32_t *d_at, hipStream_t stream);
int field_shorten_paths(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t clearance_cells,
                        const int32_t *d_paths, const int32_t *d_lengths, int32_t n_paths, int32_t max_cells, int32_t max_lookahead,
                        int32_t max_vertices, int32_t *d_vertices, int32_t *d_counts, hipStream_t stream);
}  // namespace svoslam
