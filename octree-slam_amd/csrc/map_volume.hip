// map_volume.hip -- asking the map by volume: how many occupied cells does this box hold, and how far is the nearest occupied cell
// from this point (own specification, DESIGN.md section 14: the reference has nothing like it; the restatement the device must
// equal bit for bit, `steps` included, is tests/test_volume_cpu.py).  The occupied set and the lattice are the ray cast's
// (map_query.hip, lattice.hpp); everything after the box or point has been turned into cells is integer arithmetic.
//
//   count_boxes_kernel       one box per lane.  The box becomes an inclusive cell range [lo, hi]; a cursor m runs over Morton codes
//                            (x lowest: the pool's octant order, so the octant of level l is bits 3(d-l).. of m) from morton(lo) to
//                            morton(hi).  A cursor outside the range skips the coarsest block around it that is disjoint from the
//                            range -- per axis the highest bit in which the coordinate differs from the bound it violates, by clz --
//                            which loads nothing; a cursor inside descends from the root along its path (one step), and the first
//                            node with alpha <= 127, or without children above level d, frees its whole block, so free space costs
//                            one step per block of the tree.  An occupied cell is counted; the first is the lowest in Morton order.
//   nearest_occupied_kernel  one point per lane: the same walk over the cells within `radius_cells` of the point's cell, with one
//                            more test per level of the descent, before the load: a block whose integer distance to the point's
//                            cell is not below the best squared distance so far is skipped like a free one.
//
// Both loops are flat: one `while` whose body either skips (no load) or descends, then advances the cursor past a block of 8^s
// cells -- so lanes that skip and lanes that descend share the trip count and nothing waits in an inner skip loop.  As in
// map_query.hip every step restarts at the root, a level is ONE 8-byte load, no LDS, no per-lane arrays indexed at run time.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): count_boxes_kernel 28 VGPRs, 0 bytes of scratch, occupancy
// 8; nearest_occupied_kernel 42 VGPRs, 0 bytes of scratch, occupancy 8; no LDS in either.
#include <math.h>

#include "lattice.hpp"
#include "map_descend.hpp"
#include "map_query.hpp"
#include "map_volume.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

// max(s, b), b the highest bit in which x differs from the bound of [lo, hi] it violates (-1 inside): the 2^b cells around x that
// share its higher bits all lie on x's side of that bound, the 2^(b+1) do not
__device__ inline int axis_skip_level(int x, int lo, int hi, int s) {
  const int diff = x < lo ? x ^ lo : (x > hi ? x ^ hi : 0);
  const int b = 31 - __clz(diff);  // __clz(0) == 32
  return b > s ? b : s;
}

__global__ __launch_bounds__(256) void count_boxes_kernel(const uint32_t *__restrict__ pool, const float *__restrict__ boxes, unsigned n,
                                                          int d, float cx, float cy, float cz, float h, long long stop_after,
                                                          unsigned long long *__restrict__ out_count,
                                                          unsigned long long *__restrict__ out_first_cell,
                                                          int32_t *__restrict__ out_first_node, uint32_t *__restrict__ out_steps) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int N = 1 << d;
  const float c[3] = {cx, cy, cz};
  int lo[3], hi[3];
  bool empty = false;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float mn = boxes[6 * (size_t)i + a], mx = boxes[6 * (size_t)i + 3 + a];
    if (!(mn <= mx) || mx < lattice_plane(c[a], 0, N, h) || mn > lattice_plane(c[a], N, N, h)) empty = true;  // a NaN: !(mn <= mx)
    lo[a] = cell_in_block(c[a], N, h, mn, 0, N, false);
    const int k = cell_in_block(c[a], N, h, mx, 0, N, true);
    hi[a] = k > lo[a] ? k : lo[a];
  }
  unsigned long long count = 0ull, first_cell = ~0ull;
  int32_t first_node = -1;
  uint32_t steps = 0u;
  if (!empty) {
    unsigned long long m = morton3(lo[0], lo[1], lo[2]);
    const unsigned long long mhi = morton3(hi[0], hi[1], hi[2]);
    while (m <= mhi) {
      const int x = compact3(m), y = compact3(m >> 1), z = compact3(m >> 2);
      int s = axis_skip_level(x, lo[0], hi[0], axis_skip_level(y, lo[1], hi[1], axis_skip_level(z, lo[2], hi[2], -1)));
      if (s < 0) {  // inside the range: one step
        steps++;
        uint32_t nd = 0u;
        uint2 w = make_uint2(0u, 0u);
        bool hit;
        s = d - descend<false>(pool, m, d, x, y, z, 0, 0, 0, 0, nd, w, hit);
        if (hit) {
          if (count == 0ull) {
            first_cell = (unsigned long long)x | ((unsigned long long)y << 16) | ((unsigned long long)z << 32);
            first_node = (int32_t)nd;
          }
          count++;
          if (stop_after > 0 && count == (unsigned long long)stop_after) break;
        }
      }
      m = ((m >> (3 * s)) + 1ull) << (3 * s);  // past the block of 8^s cells around m
    }
  }
  if (out_count) out_count[i] = count;
  if (out_first_cell) out_first_cell[i] = first_cell;
  if (out_first_node) out_first_node[i] = first_node;
  if (out_steps) out_steps[i] = steps;
}

__global__ __launch_bounds__(256) void nearest_occupied_kernel(const uint32_t *__restrict__ pool, const float *__restrict__ points,
                                                               unsigned n, int d, float cx, float cy, float cz, float h, int R,
                                                               int32_t *__restrict__ out_dist2, unsigned long long *__restrict__ out_cell,
                                                               int32_t *__restrict__ out_node, uint32_t *__restrict__ out_color,
                                                               uint32_t *__restrict__ out_steps) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int N = 1 << d;
  const float c[3] = {cx, cy, cz};
  int q[3], lo[3], hi[3];
  bool inside = true;
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const float p = points[3 * (size_t)i + a];
    inside = inside && lattice_plane(c[a], 0, N, h) <= p && p <= lattice_plane(c[a], N, N, h);  // false for a NaN
    q[a] = cell_in_block(c[a], N, h, p, 0, N, false);
    lo[a] = q[a] - R > 0 ? q[a] - R : 0;
    hi[a] = q[a] + R < N - 1 ? q[a] + R : N - 1;
  }
  int32_t dist2 = -2, node = -1;
  unsigned long long cell = ~0ull;
  uint32_t color = 0u, steps = 0u;
  if (inside) {
    int best = R * R + 1;
    unsigned long long m = morton3(lo[0], lo[1], lo[2]);
    const unsigned long long mhi = morton3(hi[0], hi[1], hi[2]);
    while (m <= mhi) {
      const int x = compact3(m), y = compact3(m >> 1), z = compact3(m >> 2);
      int s = axis_skip_level(x, lo[0], hi[0], axis_skip_level(y, lo[1], hi[1], axis_skip_level(z, lo[2], hi[2], -1)));
      if (s < 0) {
        steps++;
        uint32_t nd = 0u;
        uint2 w = make_uint2(0u, 0u);
        bool hit;
        s = d - descend<true>(pool, m, d, x, y, z, q[0], q[1], q[2], best, nd, w, hit);
        if (hit) {  // the prune let it through: nearer than the best so far
          const int dx = x - q[0], dy = y - q[1], dz = z - q[2];
          best = dx * dx + dy * dy + dz * dz;
          cell = (unsigned long long)x | ((unsigned long long)y << 16) | ((unsigned long long)z << 32);
          node = (int32_t)nd;
          color = w.y;
          if (best == 0) break;
        }
      }
      m = ((m >> (3 * s)) + 1ull) << (3 * s);
    }
    dist2 = node >= 0 ? best : -1;
  }
  if (out_dist2) out_dist2[i] = dist2;
  if (out_cell) out_cell[i] = cell;
  if (out_node) out_node[i] = node;
  if (out_color) out_color[i] = color;
  if (out_steps) out_steps[i] = steps;
}

}  // namespace

int pool_count_boxes(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_boxes, int64_t stop_after,
                     int32_t n, uint64_t *d_count, uint64_t *d_first_cell, int32_t *d_first_node, uint32_t *d_steps,
                     hipStream_t stream) {
  SVO_TRY(query_args(pool, depth, center, edge, d_boxes, n));
  if (n == 0) return SVOSLAM_OK;
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as pool_cast_rays drains pending asynchronous fusions
  const float h = edge / (float)(1 << depth);
  StageScope query(kStageQuery, stream);
  count_boxes_kernel<<<cdiv(n, 256), 256, 0, stream>>>(pool->d_data, d_boxes, (unsigned)n, depth, center[0], center[1], center[2], h,
                                                       (long long)stop_after, reinterpret_cast<unsigned long long *>(d_count),
                                                       reinterpret_cast<unsigned long long *>(d_first_cell), d_first_node, d_steps);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int pool_nearest_occupied(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_points,
                          int32_t radius_cells, int32_t n, int32_t *d_dist2, uint64_t *d_cell, int32_t *d_node, uint32_t *d_color,
                          uint32_t *d_steps, hipStream_t stream) {
  SVO_TRY(query_args(pool, depth, center, edge, d_points, n));
  if (radius_cells < 0 || radius_cells > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // 3 R^2 fits an int32
  if (n == 0) return SVOSLAM_OK;
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));
  const float h = edge / (float)(1 << depth);
  StageScope query(kStageQuery, stream);
  nearest_occupied_kernel<<<cdiv(n, 256), 256, 0, stream>>>(pool->d_data, d_points, (unsigned)n, depth, center[0], center[1], center[2],
                                                            h, radius_cells, d_dist2, reinterpret_cast<unsigned long long *>(d_cell),
                                                            d_node, d_color, d_steps);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
