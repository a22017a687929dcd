// map_observe.hip -- the observed space of a map region (own specification; the restatement the device must
// equal byte for byte is tests/test_observe_cpu.py).  Two calls beside the map, neither of which changes it:
//
// field_observe_rays   what a set of sensor rays has seen: per region cell a THROUGH bit (a ray passed through it) and an END bit
//                      (a ray ended in it).  It sees no pool.  The move of a point is mat4_mul_point, the cell of a coordinate
//                      cell_in_block (lattice.hpp), the cells between the two ends supercover_walk.hpp's walk -- here in its scatter
//                      form: the functor marks what the ray passes instead of testing it.
//   observe_kernel         one lane per ray, frames outermost.  The pose is read per lane (a wavefront straddles two frames where n
//                          is no multiple of 64; within a frame all lanes read the same 12 words, from cache).  A ray is classified
//                          void / outside / far / marked; the four counts are ballot popcounts, added by lane 0 with one 64-bit
//                          atomicAdd per wavefront and class that occurs.  A marked ray whose bounding box misses the region walks
//                          nothing.  Otherwise the END bit of e, the THROUGH bit of s and of every cell the walk visits are set
//                          where the cell lies in the region, in two bit planes over the region's rows (the raster's layout: one
//                          64-bit word per 64 cells of a row).  A mark is a load of the word (relaxed, agent scope: served by L2,
//                          where the atomics execute) and an atomicOr only if the bit is still clear: bits are only ever set, so a
//                          stale load costs one redundant atomic, and the rays of a frame, which all start in the sensor's cell, do
//                          not queue up on the words around it.  Keys are int64: |D| < 2^16 inside a root of depth <= 16.
//   observe_finish_kernel  one lane per region cell, x fastest: the two plane bits become the cell's byte (accumulate: ORed into
//                          it, bits 2..7 as found), and the cells whose byte then has each bit are counted: a ballot popcount per
//                          wavefront, four partial pairs through LDS, one 64-bit atomicAdd per workgroup and count.
//   The six counts are added straight into the caller's d_summary (cleared first on the stream): the record of the call is that
//   array, and without it nothing is counted.  Neither variant of section 25 (entering the walk at the region, electing one lane
//   per word) is built.
// pool_frontier_field  the observation held against the map: map_region.hip's raster of the region itself (no inflation), then
//   frontier_kernel        one lane per region cell: its occupancy bit, its byte, and for a FREE cell the bytes and bits of the six
//                          face neighbours that lie in the region.  The state and the frontier byte are stored, the six state
//                          counts are ballot popcounts summed through LDS, one 32-bit atomicAdd per workgroup and state that occurs.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 25; every kernel 0 bytes of scratch.  No
// per-lane arrays indexed at run time; every store is a vector store from plain C++.
#include <limits.h>

#include "lattice.hpp"
#include "map_observe.hpp"
#include "map_region.hpp"
#include "stage_timing.hpp"
#include "supercover_walk.hpp"

namespace svoslam {

namespace {

enum RayClass { kVoid = 0, kOutside = 1, kFar = 2, kMarked = 3 };  // the order of the summary's first four counts

// the bit of cell (x, y, z) of the region's rows
__device__ __forceinline__ bool bit_of(const unsigned long long *__restrict__ bits, int wpr, int ny, int x, int y, int z) {
  return (bits[((long long)z * ny + y) * wpr + (x >> 6)] >> (x & 63)) & 1ull;
}

// sets the bit of region cell (rx, ry, rz) in a plane that other lanes and workgroups are setting bits of
__device__ __forceinline__ void mark(unsigned long long *plane, int wpr, int ny, unsigned rx, unsigned ry, unsigned rz) {
  unsigned long long *word = plane + ((long long)rz * ny + ry) * wpr + (rx >> 6);
  const unsigned long long bit = 1ull << (rx & 63);
  if (!(__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) atomicOr(word, bit);
}

// range2: range_cells^2, or -1 for no limit.  through / end: the two planes, NULL where the region has no cells.  summary: NULL or
// the caller's six counts, cleared before this launch
__global__ __launch_bounds__(256) void observe_kernel(int N, float cx, float cy, float cz, float h, int ox, int oy, int oz, int nx, int ny,
                                                      int nz, int wpr, const float *__restrict__ points, int n, int total,
                                                      const float *__restrict__ poses, long long range2, unsigned long long *through,
                                                      unsigned long long *end, unsigned long long *summary) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  int cls = -1;                                                // a lane past the last ray counts nowhere
  if (lane_idx < (unsigned)total) {
    const int i = (int)lane_idx;
    const float *__restrict__ m = poses + 16 * (size_t)(i / n);  // per lane: the wavefront may hold the end of one frame and the start of the next
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    cls = kVoid;
    if (finitef_(px) && finitef_(py) && finitef_(pz)) {
      cls = kOutside;
      const float c[3] = {cx, cy, cz};
      const float o[3] = {m[12], m[13], m[14]};
      float w[3];
      mat4_mul_point(m, px, py, pz, 1.0f, w[0], w[1], w[2]);
      bool inside = true;
      int s[3], e[3];
#pragma unroll
      for (int a = 0; a < 3; a++) {
        const float lo = lattice_plane(c[a], 0, N, h), hi = lattice_plane(c[a], N, N, h);
        inside = inside && finitef_(o[a]) && finitef_(w[a]) && lo <= o[a] && o[a] <= hi && lo <= w[a] && w[a] <= hi;
        s[a] = cell_in_block(c[a], N, h, o[a], 0, N, false);
        e[a] = cell_in_block(c[a], N, h, w[a], 0, N, false);
      }
      if (inside) {
        const long long dx = e[0] - s[0], dy = e[1] - s[1], dz = e[2] - s[2];
        if (range2 >= 0 && dx * dx + dy * dy + dz * dz > range2) {
          cls = kFar;
        } else {
          cls = kMarked;
          // the cells of the ray lie in the bounding box of s and e: a box that misses the region marks nothing
          const bool meets = through && max(s[0], e[0]) >= ox && min(s[0], e[0]) < ox + nx && max(s[1], e[1]) >= oy &&
                             min(s[1], e[1]) < oy + ny && max(s[2], e[2]) >= oz && min(s[2], e[2]) < oz + nz;
          if (meets) {
            const unsigned ex = (unsigned)(e[0] - ox), ey = (unsigned)(e[1] - oy), ez = (unsigned)(e[2] - oz);
            if (ex < (unsigned)nx && ey < (unsigned)ny && ez < (unsigned)nz) mark(end, wpr, ny, ex, ey, ez);
            if (dx | dy | dz) {
              const unsigned sx = (unsigned)(s[0] - ox), sy = (unsigned)(s[1] - oy), sz = (unsigned)(s[2] - oz);
              if (sx < (unsigned)nx && sy < (unsigned)ny && sz < (unsigned)nz) mark(through, wpr, ny, sx, sy, sz);
              supercover_walk<long long>(s[0], s[1], s[2], dx, dy, dz, [&](int x, int y, int z) {
                const unsigned rx = (unsigned)(x - ox), ry = (unsigned)(y - oy), rz = (unsigned)(z - oz);
                if (rx < (unsigned)nx && ry < (unsigned)ny && rz < (unsigned)nz) mark(through, wpr, ny, rx, ry, rz);
                return false;
              });
            }
          }
        }
      }
    }
  }
  if (!summary) return;  // uniform
  const int n_void = __popcll(__ballot(cls == kVoid)), n_outside = __popcll(__ballot(cls == kOutside));
  const int n_far = __popcll(__ballot(cls == kFar)), n_marked = __popcll(__ballot(cls == kMarked));
  if ((threadIdx.x & 63) == 0) {
    if (n_void) atomicAdd(&summary[kVoid], (unsigned long long)n_void);
    if (n_outside) atomicAdd(&summary[kOutside], (unsigned long long)n_outside);
    if (n_far) atomicAdd(&summary[kFar], (unsigned long long)n_far);
    if (n_marked) atomicAdd(&summary[kMarked], (unsigned long long)n_marked);
  }
}

__global__ __launch_bounds__(256) void observe_finish_kernel(const unsigned long long *__restrict__ through,
                                                             const unsigned long long *__restrict__ end, int wpr, int nx, int total,
                                                             int accumulate, uint8_t *__restrict__ obs, unsigned long long *summary) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  unsigned v = 0u;
  if (lane_idx < (unsigned)total) {
    const int idx = (int)lane_idx, x = idx % nx;
    const long long word = (long long)(idx / nx) * wpr + (x >> 6);
    const unsigned marks = (unsigned)((through[word] >> (x & 63)) & 1ull) * SVOSLAM_OBS_THROUGH +
                           (unsigned)((end[word] >> (x & 63)) & 1ull) * SVOSLAM_OBS_END;
    if (accumulate) {
      const unsigned before = obs[idx];
      v = before | marks;
      if (v != before) obs[idx] = (uint8_t)v;
    } else {
      v = marks;
      obs[idx] = (uint8_t)v;
    }
  }
  if (!summary) return;  // uniform
  const int n_through = __popcll(__ballot((v & SVOSLAM_OBS_THROUGH) != 0u)), n_end = __popcll(__ballot((v & SVOSLAM_OBS_END) != 0u));
  __shared__ int part[4][2];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = n_through;
    part[threadIdx.x >> 6][1] = n_end;
  }
  __syncthreads();
  if (threadIdx.x < 2) {
    const int sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&summary[4 + threadIdx.x], (unsigned long long)sum);
  }
}

// neither occupied nor marked: what a FREE cell beside it is a frontier for
__device__ __forceinline__ bool unknown_at(const unsigned long long *__restrict__ bits, int wpr, int ny, const uint8_t *__restrict__ obs,
                                           int x, int y, int z, int idx) {
  return !(obs[idx] & (SVOSLAM_OBS_THROUGH | SVOSLAM_OBS_END)) && !bit_of(bits, wpr, ny, x, y, z);
}

// bits: the occupancy rows of the region itself
__global__ __launch_bounds__(256) void frontier_kernel(const unsigned long long *__restrict__ bits, int wpr, int nx, int ny, int nz,
                                                       int total, const uint8_t *__restrict__ obs, uint8_t *__restrict__ state,
                                                       uint8_t *__restrict__ frontier, int32_t *summary) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  int st = -1;                                                 // a lane past the last cell counts nowhere
  if (lane_idx < (unsigned)total) {
    const int idx = (int)lane_idx;
    const int x = idx % nx, y = (idx / nx) % ny, z = idx / nx / ny;
    const unsigned own = obs[idx];
    const bool t = (own & SVOSLAM_OBS_THROUGH) != 0u, e = (own & SVOSLAM_OBS_END) != 0u;
    if (bit_of(bits, wpr, ny, x, y, z)) {
      st = t && !e ? SVOSLAM_STATE_VACATED : SVOSLAM_STATE_OCCUPIED;
    } else if (e) {
      st = SVOSLAM_STATE_UNMAPPED;
    } else if (!t) {
      st = SVOSLAM_STATE_UNKNOWN;
    } else {  // a neighbour outside the region never makes a frontier
      const int row = nx, plane = nx * ny;
      bool beside = x > 0 && unknown_at(bits, wpr, ny, obs, x - 1, y, z, idx - 1);
      beside = beside || (x + 1 < nx && unknown_at(bits, wpr, ny, obs, x + 1, y, z, idx + 1));
      beside = beside || (y > 0 && unknown_at(bits, wpr, ny, obs, x, y - 1, z, idx - row));
      beside = beside || (y + 1 < ny && unknown_at(bits, wpr, ny, obs, x, y + 1, z, idx + row));
      beside = beside || (z > 0 && unknown_at(bits, wpr, ny, obs, x, y, z - 1, idx - plane));
      beside = beside || (z + 1 < nz && unknown_at(bits, wpr, ny, obs, x, y, z + 1, idx + plane));
      st = beside ? SVOSLAM_STATE_FRONTIER : SVOSLAM_STATE_FREE;
    }
    if (state) state[idx] = (uint8_t)st;
    if (frontier) frontier[idx] = st == SVOSLAM_STATE_FRONTIER ? 1 : 0;
  }
  if (!summary) return;  // uniform
  const int n0 = __popcll(__ballot(st == 0)), n1 = __popcll(__ballot(st == 1)), n2 = __popcll(__ballot(st == 2));
  const int n3 = __popcll(__ballot(st == 3)), n4 = __popcll(__ballot(st == 4)), n5 = __popcll(__ballot(st == 5));
  __shared__ int part[4][6];
  if ((threadIdx.x & 63) == 0) {
    const int wave = threadIdx.x >> 6;
    part[wave][0] = n0; part[wave][1] = n1; part[wave][2] = n2;
    part[wave][3] = n3; part[wave][4] = n4; part[wave][5] = n5;
  }
  __syncthreads();
  if (threadIdx.x < 6) {
    const int sum = part[0][threadIdx.x] + part[1][threadIdx.x] + part[2][threadIdx.x] + part[3][threadIdx.x];
    if (sum) atomicAdd(&summary[threadIdx.x], sum);
  }
}

int observe(svoslam_workspace *ws, uint8_t *d_obs, int depth, const float center[3], float edge, const int32_t origin[3],
            const int32_t dims[3], long long cells, long long wpr, long long words, const float *d_points, int n, long long rays,
            const float *d_poses, int range_cells, int accumulate, int64_t *d_summary, hipStream_t stream) {
  unsigned long long *through = nullptr, *end = nullptr, *summary = reinterpret_cast<unsigned long long *>(d_summary);
  if (cells > 0) {  // the one allocation comes before anything is written
    SVO_TRY(ws->obs_bits.reserve((size_t)words * 16));
    through = ws->obs_bits.as<unsigned long long>();
    end = through + words;
    SVO_HIP(hipMemsetAsync(through, 0, (size_t)words * 16, stream));
  }
  if (summary) SVO_HIP(hipMemsetAsync(summary, 0, 6 * sizeof(unsigned long long), stream));
  if (rays > 0 && (cells > 0 || summary)) {
    const int N = 1 << depth;
    const long long range2 = range_cells > 0 ? (long long)range_cells * range_cells : -1;
    observe_kernel<<<cdiv(rays, 256), 256, 0, stream>>>(N, center[0], center[1], center[2], edge / (float)N, origin[0], origin[1], origin[2],
                                                        dims[0], dims[1], dims[2], (int)wpr, d_points, n, (int)rays, d_poses, range2,
                                                        through, end, summary);
    SVO_LAUNCH_CHECK();
  }
  if (cells > 0) {
    observe_finish_kernel<<<cdiv(cells, 256), 256, 0, stream>>>(through, end, (int)wpr, dims[0], (int)cells, accumulate, d_obs, summary);
    SVO_LAUNCH_CHECK();
  }
  return SVOSLAM_OK;
}

}  // namespace

int field_observe_rays(svoslam_workspace *ws, uint8_t *d_obs, int depth, const float center[3], float edge, const int32_t origin[3],
                       const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, int32_t n_frames, int32_t range_cells,
                       int32_t accumulate, int64_t *d_summary, hipStream_t stream) {
  if (!ws || !center || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH || !(edge > 0.0f)) return SVOSLAM_ERR_INVALID_ARG;
  const long long N = 1ll << depth;
  long long cells = 1;  // every side is <= 2^16: no overflow
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > N) return SVOSLAM_ERR_INVALID_ARG;
    cells *= dims[a];
  }
  if (n < 0 || n_frames < 0 || range_cells < 0 || range_cells > (1 << SVOSLAM_MAX_DEPTH)) return SVOSLAM_ERR_INVALID_ARG;
  const long long rays = (long long)n * n_frames;
  if ((cells > 0 && !d_obs) || (rays > 0 && (!d_points || !d_poses))) return SVOSLAM_ERR_INVALID_ARG;
  if (cells > (long long)INT_MAX) {
    set_last_error_text("svoslam_field_observe_rays: %d x %d x %d cells are more than 2^31 - 1", dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (rays > (long long)INT_MAX) {
    set_last_error_text("svoslam_field_observe_rays: %d frames of %d rays are more than 2^31 - 1", n_frames, n);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  const long long wpr = ((long long)dims[0] + 63) / 64, words = cells > 0 ? wpr * dims[1] * dims[2] : 0;  // words <= cells
  SlotRollback grown({&ws->obs_bits});
  StageScope query(kStageQuery, stream);
  const int rc = observe(ws, d_obs, depth, center, edge, origin, dims, cells, wpr, words, d_points, n, rays, d_poses, range_cells,
                         accumulate, d_summary, stream);
  return rc == SVOSLAM_OK ? rc : grown.undo(rc, stream);
}

int pool_frontier_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                        const uint8_t *d_obs, uint8_t *d_state, uint8_t *d_frontier, int32_t *d_summary, hipStream_t stream) {
  if (!ws || (!d_state && !d_frontier && !d_summary)) return SVOSLAM_ERR_INVALID_ARG;
  RegionPlan p;  // the region itself: a neighbour outside it is never read
  SVO_TRY(plan_region(depth, origin, dims, 0, &p));
  if (p.nothing) {  // no cells: every state counts none
    if (!d_summary) return SVOSLAM_OK;
    StageScope query(kStageQuery, stream);
    SVO_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int32_t), stream));
    return SVOSLAM_OK;
  }
  if (!d_obs) return SVOSLAM_ERR_INVALID_ARG;
  SVO_TRY(admit_region("svoslam_pool_frontier_field", pool, p, 0, false, stream));
  SlotRollback grown({&ws->front_bits});
  const int rc = ws->front_bits.reserve((size_t)p.words * 8);
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  unsigned long long *bits = ws->front_bits.as<unsigned long long>();
  StageScope query(kStageQuery, stream);
  if (d_summary) SVO_HIP(hipMemsetAsync(d_summary, 0, 6 * sizeof(int32_t), stream));
  SVO_TRY(region_raster(pool, depth, p, false, bits, stream));
  frontier_kernel<<<cdiv(p.n_out, 256), 256, 0, stream>>>(bits, (int)p.wpr, (int)p.nx, (int)p.ny, (int)p.nz, (int)p.n_out, d_obs, d_state,
                                                          d_frontier, d_summary);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
