// map_corridor.hpp -- safe corridors over a distance field: boxes of free cells grown layer by layer, and the chain of them that
// holds a planned path (map_corridor.hip; own specification, include/svoslam_corridor.h and DESIGN.md section 27).
//
// d_dist2 is a field as svoslam_pool_distance_field writes it.  Neither call can check the field's radius: the caller must supply one
// computed with a radius >= clearance_cells, or cells nearer than that pass for free.  A region has at most 2^16 cells per axis and
// 2^31 - 1 in all, as for map_paths.hpp.  The two extern "C" entries are in map_corridor.hip as well.
#pragma once
#include "../../include/svoslam_corridor.h"
#include "common.hpp"

namespace svoslam {
int field_grow_boxes(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t clearance_cells, int32_t max_extent,
                     const int32_t *d_seeds, int32_t n, int32_t *d_boxes, int32_t *d_layers, hipStream_t stream);
int field_path_corridors(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t clearance_cells,
                         int32_t max_extent, const int32_t *d_paths, const int32_t *d_lengths, int32_t n_paths, int32_t max_cells,
                         int32_t max_boxes, int32_t *d_boxes, int32_t *d_anchors, int32_t *d_counts, int32_t *d_gaps, hipStream_t stream);
}  // namespace svoslam
