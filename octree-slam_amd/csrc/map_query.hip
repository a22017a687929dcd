// map_query.hip -- asking the map: what does this ray hit first, and which node holds this point (own specification, DESIGN.md
// section 13: the reference has nothing like it; the restatement the device must equal bit for bit is tests/test_query_cpu.py).
//
//   cast_rays_kernel     one ray per lane.  The ray walks the cells of the 2^d lattice the surface mesh is built on (section 12):
//                        plane k of an axis is center + (float)(2k - N) * (edge / (float)N), a plane's parameter is
//                        (plane - o) * (1.0f / v), every product and sum rounded on its own (the unit is compiled with
//                        contraction off, common.hpp).  A step descends from the root along the current cell's path; the first node
//                        with alpha <= 127, or without children above level d, frees its whole aligned block, which the ray leaves
//                        through the nearest of its (at most three) leaving planes -- so free space costs one step per block of the
//                        tree, not per cell.  The other two coordinates are recounted by comparison against the planes of the block
//                        (a binary search of d - level probes, none for a block of one cell) and never move backwards.
//   query_points_kernel  one point per lane: the fusion's own descent (computeKey, svo.cu:63-90: octant bits from p > c, the edge
//                        halved, the centre moved by +-edge) to max_depth or the first childless node.
//
// Every step restarts at the root: model_depth.hip measured that resuming at a kept node is slower here (the upper levels are cache
// hits, the extra registers cost more).  A level is ONE 8-byte load (children word and colour word together), so the dependent
// chain of a descent is one load and one wait per level; the loop is divergent in its trip count and in nothing else that costs,
// so its body is kept short: planes are computed, not tabulated, no LDS, no per-lane arrays indexed at run time.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): cast_rays_kernel 39 VGPRs, 0 bytes of scratch, occupancy 8;
// query_points_kernel 18 VGPRs, 0 bytes of scratch, occupancy 8.
#include <math.h>

#include "lattice.hpp"
#include "map_query.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

__global__ __launch_bounds__(256) void cast_rays_kernel(const uint32_t *__restrict__ pool, const float *__restrict__ rays,
                                                        const float *__restrict__ t_max, unsigned n, int d, float cx, float cy, float cz,
                                                        float h, float *__restrict__ out_t, int32_t *__restrict__ out_node,
                                                        unsigned long long *__restrict__ out_cell, uint32_t *__restrict__ out_color,
                                                        uint32_t *__restrict__ out_steps) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const int N = 1 << d;
  const float c[3] = {cx, cy, cz};
  float o[3], v[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    o[a] = rays[6 * (size_t)i + a];
    v[a] = rays[6 * (size_t)i + 3 + a];
  }
  const float tmax = t_max ? t_max[i] : INFINITY;
  float t = NAN;
  int32_t node = -1;
  unsigned long long cell = ~0ull;
  uint32_t color = 0u, steps = 0u;
  const bool valid = finitef_(o[0]) && finitef_(o[1]) && finitef_(o[2]) && finitef_(v[0]) && finitef_(v[1]) && finitef_(v[2]) &&
                     (v[0] != 0.0f || v[1] != 0.0f || v[2] != 0.0f);
  if (valid) {
    t = INFINITY;  // a miss until a cell is hit
    float r[3];
    bool inside = true;
#pragma unroll
    for (int a = 0; a < 3; a++) {
      r[a] = v[a] != 0.0f ? 1.0f / v[a] : 0.0f;
      inside = inside && lattice_plane(c[a], 0, N, h) <= o[a] && o[a] <= lattice_plane(c[a], N, N, h);
    }
    int q[3] = {0, 0, 0}, face = 6;
    float tc = 0.0f;  // the parameter the current cell was entered at
    bool live = true;
    if (inside) {
#pragma unroll
      for (int a = 0; a < 3; a++) q[a] = cell_in_block(c[a], N, h, o[a], 0, N, v[a] < 0.0f);
    } else {
      float te = -INFINITY, tf = INFINITY;
      int ax = -1;
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float p0 = lattice_plane(c[a], 0, N, h), pn = lattice_plane(c[a], N, N, h);
        if (v[a] != 0.0f) {
          const float tn = ((v[a] > 0.0f ? p0 : pn) - o[a]) * r[a], tx = ((v[a] > 0.0f ? pn : p0) - o[a]) * r[a];
          if (tn > te) { te = tn; ax = a; }  // the lowest axis that attains the largest
          if (tx < tf) tf = tx;
        } else if (!(p0 <= o[a] && o[a] <= pn)) {
          live = false;
        }
      }
      if (ax < 0 || te < 0.0f || te > tf) live = false;
      if (live) {
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (a == ax) {
            q[a] = v[a] > 0.0f ? 0 : N - 1;
            face = 2 * a + (v[a] > 0.0f ? 0 : 1);
          } else {
            q[a] = cell_in_block(c[a], N, h, o[a] + te * v[a], 0, N, v[a] < 0.0f);
          }
        }
        tc = te;
      }
    }
    if (live && tc > tmax) live = false;
    if (live) {
      for (int step = 0; step < 3 * N; step++) {  // every coordinate is monotone and one advances: at most 3N blocks
        steps++;
        uint32_t child = 0u, nd = 0u;
        uint2 w = make_uint2(0u, 0u);
        int l = 1;
        bool hit = false;
        for (;; l++) {
          const int sh = d - l;
          nd = child + ((((uint32_t)q[0] >> sh) & 1u) | ((((uint32_t)q[1] >> sh) & 1u) << 1) | ((((uint32_t)q[2] >> sh) & 1u) << 2));
          w = *reinterpret_cast<const uint2 *>(pool + 2 * (size_t)nd);
          if ((w.y >> 24) <= 127u) break;
          if (l == d) { hit = true; break; }
          if (!(w.x & kFlag)) break;
          child = w.x & kMask;
        }
        if (hit) {
          t = tc;
          node = (int32_t)nd;
          color = w.y;
          cell = (unsigned long long)q[0] | ((unsigned long long)q[1] << 16) | ((unsigned long long)q[2] << 32) |
                 ((unsigned long long)face << 48);
          break;
        }
        // the block of level l is free: leave it through the nearest leaving plane, the lowest axis on a tie
        const int sh = d - l, size = 1 << sh;
        float tl = INFINITY;
        int ax = -1;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          if (v[a] != 0.0f) {
            const int lo = (q[a] >> sh) << sh;
            const float tp = (lattice_plane(c[a], v[a] > 0.0f ? lo + size : lo, N, h) - o[a]) * r[a];
            if (tp < tl) { tl = tp; ax = a; }
          }
        }
        if (ax < 0) break;  // no plane is ever reached
        bool left = false;
#pragma unroll
        for (int a = 0; a < 3; a++) {
          const int lo = (q[a] >> sh) << sh;
          if (a == ax) {
            q[a] = v[a] > 0.0f ? lo + size : lo - 1;
            face = 2 * a + (v[a] > 0.0f ? 0 : 1);
            left = q[a] < 0 || q[a] >= N;
          } else {
            const int k = cell_in_block(c[a], N, h, o[a] + tl * v[a], lo, size, v[a] < 0.0f);
            q[a] = v[a] > 0.0f ? (k > q[a] ? k : q[a]) : (v[a] < 0.0f ? (k < q[a] ? k : q[a]) : k);
          }
        }
        if (left) break;
        tc = tl > tc ? tl : tc;
        if (tc > tmax) break;
      }
    }
  }
  if (out_t) out_t[i] = t;
  if (out_node) out_node[i] = node;
  if (out_cell) out_cell[i] = cell;
  if (out_color) out_color[i] = color;
  if (out_steps) out_steps[i] = steps;
}

__global__ __launch_bounds__(256) void query_points_kernel(const uint32_t *__restrict__ pool, const float *__restrict__ points, unsigned n,
                                                           int depth, float cx, float cy, float cz, float edge,
                                                           int32_t *__restrict__ out_node, int32_t *__restrict__ out_level,
                                                           unsigned long long *__restrict__ out_key, uint32_t *__restrict__ out_color) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
  int32_t node = -1, level = 0;
  unsigned long long key = 0ull;
  uint32_t color = 0u;
  if (cx - edge <= px && px <= cx + edge && cy - edge <= py && py <= cy + edge && cz - edge <= pz && pz <= cz + edge) {
    uint32_t child = 0u;
    key = 1ull;
    for (;;) {
      const bool x = px > cx, y = py > cy, z = pz > cz;
      const uint32_t oct = (x ? 1u : 0u) + (y ? 2u : 0u) + (z ? 4u : 0u);
      node = (int32_t)(child + oct);
      key = (key << 3) + oct;
      level++;
      const uint2 w = *reinterpret_cast<const uint2 *>(pool + 2 * (size_t)node);
      color = w.y;
      if (level == depth || !(w.x & kFlag)) break;
      child = w.x & kMask;
      edge = edge / 2.0f;
      cx += x ? edge : -edge;  // edge * (+-1): exact
      cy += y ? edge : -edge;
      cz += z ? edge : -edge;
    }
  }
  if (out_node) out_node[i] = node;
  if (out_level) out_level[i] = level;
  if (out_key) out_key[i] = key;
  if (out_color) out_color[i] = color;
}

}  // namespace

int query_args(const svoslam_pool *pool, int depth, const float center[3], float edge, const void *d_in, int32_t n) {
  if (n < 0 || depth < 1 || depth > SVOSLAM_MAX_DEPTH || !(edge > 0.0f) || !center) return SVOSLAM_ERR_INVALID_ARG;
  if (n > 0 && (!pool || !pool->d_data || !d_in)) return SVOSLAM_ERR_INVALID_ARG;
  return SVOSLAM_OK;
}

int pool_cast_rays(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_rays, const float *d_t_max,
                   int32_t n, float *d_t, int32_t *d_node, uint64_t *d_cell, uint32_t *d_color, uint32_t *d_steps, hipStream_t stream) {
  SVO_TRY(query_args(pool, depth, center, edge, d_rays, n));
  if (n == 0) return SVOSLAM_OK;
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as extract_voxel_grid drains pending asynchronous fusions
  const float h = edge / (float)(1 << depth);
  StageScope query(kStageQuery, stream);
  cast_rays_kernel<<<cdiv(n, 256), 256, 0, stream>>>(pool->d_data, d_rays, d_t_max, (unsigned)n, depth, center[0], center[1], center[2], h,
                                                     d_t, d_node, reinterpret_cast<unsigned long long *>(d_cell), d_color, d_steps);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int pool_query_points(const svoslam_pool *pool, int depth, const float center[3], float edge, const float *d_points, int32_t n,
                      int32_t *d_node, int32_t *d_level, uint64_t *d_key, uint32_t *d_color, hipStream_t stream) {
  SVO_TRY(query_args(pool, depth, center, edge, d_points, n));
  if (n == 0) return SVOSLAM_OK;
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));
  StageScope query(kStageQuery, stream);
  query_points_kernel<<<cdiv(n, 256), 256, 0, stream>>>(pool->d_data, d_points, (unsigned)n, depth, center[0], center[1], center[2], edge,
                                                        d_node, d_level, reinterpret_cast<unsigned long long *>(d_key), d_color);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
