// map_query.hpp -- asking the map: exact ray casting against the occupied set and batched point lookup (map_query.hip; own
// specification)
#pragma once
#include "common.hpp"

namespace svoslam {
// the argument check every map query shares (map_volume.hip too): see the errors listed in include/svoslam.h
int query_args(const svoslam_pool *pool, int depth, const float center[3], float edge, const void *d_in, int32_t n);
int pool_cast_rays(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_rays, const float *d_t_max,
                   int32_t n, float *d_t, int32_t *d_node, uint64_t *d_cell, uint32_t *d_color, uint32_t *d_steps, hipStream_t stream);
int pool_query_points(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_points, int32_t n,
                      int32_t *d_node, int32_t *d_level, uint64_t *d_key, uint32_t *d_color, hipStream_t stream);
}  // namespace svoslam
