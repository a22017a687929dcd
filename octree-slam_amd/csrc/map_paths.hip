// map_paths.hip -- straightening planned paths by line of sight without giving up their clearance (own specification, DESIGN.md
// section 22: the reference has nothing like it; the restatements the device must equal value for value are in
// tests/test_paths_cpu.py).  Both calls read a distance field as svoslam_pool_distance_field writes it and take no pool and no
// workspace.  g(c) = the field's value at c, +infinity (INT_MAX here) where it is -1, 0 for a cell outside the region.
//
//   segment_clearance_kernel  one lane per segment: the minimum of g over a, the supercover of the segment in walk order, b, and
//                             the first cell that attains it.  The walk (supercover_walk.hpp) leaves only when 0 was reached, which
//                             every cell outside the region gives: no cell outside the region is ever read, and a walk that begins
//                             inside it ends at the latest one cell beyond it.  An end outside the region can be anywhere in int32:
//                             the keys are then 128-bit (chosen per lane by |D|), otherwise int64.
//   shorten_paths_kernel      one wavefront per path, the anchor a uniform.  Candidates j go up from a + 2 in batches of 64, one
//                             per lane: g(p_j) is loaded, m(a, j) is a wave min-scan (__shfl_up, six steps) with a carry across
//                             the batches, the lane walks the segment p_a .. p_j and leaves at the first cell below max(r^2 + 1, m),
//                             a ballot gives the highest admissible lane.  Admissibility is not monotone in j, so the window is
//                             scanned to its end and the best of all batches kept.  A lane walks only when both ends have g > r^2,
//                             so both lie in the region and int64 keys do (at most 2^16 cells per axis, checked on the host).
// Every device loop ends by its own data: the anchor rises strictly and stays below L, a batch loop runs to the window's end, a walk
// makes at most |D_x| + |D_y| + |D_z| crossings.  Unlimited lookahead is O(L^2) walks per path in the worst case; max_lookahead
// bounds it by L * W.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): segment_clearance_kernel 64 VGPRs / 70 SGPRs, occupancy 8;
// shorten_paths_kernel 53 VGPRs / 106 SGPRs, occupancy 7; both 0 bytes of scratch, no LDS.  No per-lane arrays indexed at run time,
// no inline assembly, plain vector stores.
#include <limits.h>

#include "map_paths.hpp"
#include "stage_timing.hpp"
#include "supercover_walk.hpp"

namespace svoslam {

namespace {

constexpr int kInfinite = INT_MAX;  // g where the field says "none within the radius"

struct FieldView {  // the region's field; a cell is addressed relative to the region's first cell
  const int32_t *__restrict__ dist2;
  int nx, ny, nz;
  // g of a cell given relative to the region: nothing outside the region is read
  __device__ __forceinline__ int g(long long x, long long y, long long z) const {
    if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) return 0;
    const int v = dist2[(z * ny + y) * nx + x];
    return v < 0 ? kInfinite : v;
  }
};

__global__ __launch_bounds__(256) void segment_clearance_kernel(FieldView f, int ox, int oy, int oz, const int32_t *__restrict__ segments,
                                                                int n, int32_t *__restrict__ out_min, int32_t *__restrict__ out_at) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // n <= 2^31 - 1: the sum can pass it, compared unsigned
  if (lane_idx >= (unsigned)n) return;
  const int32_t *seg = segments + 6ll * lane_idx;
  const int ax = seg[0], ay = seg[1], az = seg[2], bx = seg[3], by = seg[4], bz = seg[5];
  const long long rx = (long long)ax - ox, ry = (long long)ay - oy, rz = (long long)az - oz;
  int best = f.g(rx, ry, rz);
  int tx = ax, ty = ay, tz = az;  // the first cell that attains `best`, absolute
  if (best > 0) {                 // a lies in the region: rx, ry, rz are below 2^16
    const long long dx = (long long)bx - ax, dy = (long long)by - ay, dz = (long long)bz - az;
    auto visit = [&](int x, int y, int z) {
      const int v = f.g(x, y, z);
      if (v < best) { best = v; tx = x + ox; ty = y + oy; tz = z + oz; }
      return best == 0;
    };
    const bool narrow = walk_fits_int64(dx < 0 ? -dx : dx, dy < 0 ? -dy : dy, dz < 0 ? -dz : dz);
    const bool ended = narrow ? supercover_walk<long long>((int)rx, (int)ry, (int)rz, dx, dy, dz, visit)
                              : supercover_walk<__int128>((int)rx, (int)ry, (int)rz, dx, dy, dz, visit);
    if (!ended) {
      const int v = f.g(rx + dx, ry + dy, rz + dz);
      if (v < best) { best = v; tx = bx; ty = by; tz = bz; }
    }
  }
  out_min[lane_idx] = best == kInfinite ? -1 : best;
  if (out_at) {
    int32_t *at = out_at + 3ll * lane_idx;
    at[0] = tx; at[1] = ty; at[2] = tz;
  }
}

__global__ __launch_bounds__(256) void shorten_paths_kernel(FieldView f, int ox, int oy, int oz, int r2, const int32_t *__restrict__ paths,
                                                            const int32_t *__restrict__ lengths, int n_paths, int max_cells, int W,
                                                            int max_vertices, int32_t *__restrict__ vertices,
                                                            int32_t *__restrict__ counts) {
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // n_paths <= 2^31 - 1, compared unsigned
  if (wave >= (unsigned)n_paths) return;
  const int lane = threadIdx.x & 63;
  const long long stored = __builtin_amdgcn_readfirstlane(lengths[wave]);
  const int L = (int)min(stored < 0 ? -stored : stored, (long long)max_cells);
  const int32_t *__restrict__ cells = paths + (long long)wave * max_cells * 3;
  int32_t *__restrict__ out = vertices + (long long)wave * max_vertices;
  int count = 0;
  if (L > 0) {
    if (lane == 0 && max_vertices > 0) out[0] = 0;
    count = 1;
    int a = 0;
    while (a < L - 1) {  // a rises by at least 1 per pass
      const int px = cells[3 * a], py = cells[3 * a + 1], pz = cells[3 * a + 2];
      const long long rx = (long long)px - ox, ry = (long long)py - oy, rz = (long long)pz - oz;
      const int ga = f.g(rx, ry, rz);
      int best = a + 1;  // always admissible
      const int hi = W > 0 ? (int)min((long long)L - 1, (long long)a + W) : L - 1;
      if (ga > r2 && a + 2 <= hi) {  // otherwise a itself fails every longer shortcut; g > r^2 >= 0: a lies in the region
        const int nx1 = cells[3 * a + 3], ny1 = cells[3 * a + 4], nz1 = cells[3 * a + 5];
        int carry = min(ga, f.g((long long)nx1 - ox, (long long)ny1 - oy, (long long)nz1 - oz));  // m(a, a + 1)
        for (int base = a + 2; base <= hi; base += 64) {  // base + 63 < 2^31: L * 3 <= 2^31 - 1
          const int j = base + lane;
          const bool valid = j <= hi;
          int qx = px, qy = py, qz = pz, gj = kInfinite;
          if (valid) {
            qx = cells[3 * j]; qy = cells[3 * j + 1]; qz = cells[3 * j + 2];
            gj = f.g((long long)qx - ox, (long long)qy - oy, (long long)qz - oz);
          }
          int m = gj;  // inclusive min-scan over the lanes, then the batches before
          for (int d = 1; d < 64; d <<= 1) {
            const int below = __shfl_up(m, d);
            if (lane >= d) m = min(m, below);
          }
          m = min(m, carry);
          carry = __shfl(m, 63);
          bool ok = valid && gj > r2;  // then p_j lies in the region too, and |D| is below 2^16 per axis
          if (ok) {
            const int floor_g = max(r2 + 1, m);
            ok = !supercover_walk<long long>((int)rx, (int)ry, (int)rz, (long long)qx - px, (long long)qy - py, (long long)qz - pz,
                                             [&](int x, int y, int z) { return f.g(x, y, z) < floor_g; });
          }
          const unsigned long long admissible = __ballot(ok);
          if (admissible) best = base + 63 - __clzll((long long)admissible);  // later batches hold larger j
        }
      }
      a = best;
      if (lane == 0 && count < max_vertices) out[count] = a;
      count++;
    }
  }
  if (lane == 0) counts[wave] = count;
}

// the checks both calls share: the region's size.  -> SVOSLAM_OK with *cells set
int region_cells(const char *who, const int32_t dims[3], long long *cells) {
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  const long long plane = empty ? 0 : (long long)dims[0] * dims[1];  // below 2^62; the third factor only after it was tested
  *cells = plane > INT_MAX ? plane : plane * dims[2];
  if (*cells > INT_MAX) {
    set_last_error_text("%s: %d x %d x %d cells are more than 2^31 - 1", who, dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (!empty && (dims[0] > kWalkMaxAxisCells || dims[1] > kWalkMaxAxisCells || dims[2] > kWalkMaxAxisCells)) {
    set_last_error_text("%s: %d x %d x %d cells are more than 2^16 along an axis, the bound of the walk's keys", who, dims[0], dims[1],
                        dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  return SVOSLAM_OK;
}

}  // namespace

int field_segment_clearance(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], const int32_t *d_segments, int32_t n,
                            int32_t *d_min, int32_t *d_at, hipStream_t stream) {
  if (!origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n < 0) return SVOSLAM_ERR_INVALID_ARG;
  long long cells;
  SVO_TRY(region_cells("svoslam_field_segment_clearance", dims, &cells));
  if (n == 0) return SVOSLAM_OK;
  if (!d_segments || !d_min || (cells > 0 && !d_dist2)) return SVOSLAM_ERR_INVALID_ARG;
  const FieldView f = {d_dist2, cells ? dims[0] : 0, cells ? dims[1] : 0, cells ? dims[2] : 0};
  StageScope timed(kStageQuery, stream);
  segment_clearance_kernel<<<cdiv(n, 256), 256, 0, stream>>>(f, origin[0], origin[1], origin[2], d_segments, n, d_min, d_at);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int field_shorten_paths(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t r, const int32_t *d_paths,
                        const int32_t *d_lengths, int32_t n_paths, int32_t max_cells, int32_t max_lookahead, int32_t max_vertices,
                        int32_t *d_vertices, int32_t *d_counts, hipStream_t stream) {
  if (!origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n_paths < 0 || max_cells < 0 || max_lookahead < 0 ||
      max_vertices < 0 || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS)
    return SVOSLAM_ERR_INVALID_ARG;
  long long cells;
  SVO_TRY(region_cells("svoslam_field_shorten_paths", dims, &cells));
  if ((long long)n_paths * max_cells > INT_MAX / 3) {
    set_last_error_text("svoslam_field_shorten_paths: %d paths of %d cells are more than 2^31 - 1 path entries", n_paths, max_cells);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if ((long long)n_paths * max_vertices > INT_MAX) {
    set_last_error_text("svoslam_field_shorten_paths: %d paths of %d vertices are more than 2^31 - 1 entries", n_paths, max_vertices);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_paths == 0) return SVOSLAM_OK;
  if (!d_lengths || !d_counts || (cells > 0 && !d_dist2) || (max_cells > 0 && !d_paths) || (max_vertices > 0 && !d_vertices))
    return SVOSLAM_ERR_INVALID_ARG;
  const FieldView f = {d_dist2, cells ? dims[0] : 0, cells ? dims[1] : 0, cells ? dims[2] : 0};
  StageScope timed(kStageQuery, stream);
  shorten_paths_kernel<<<cdiv(n_paths, 4), 256, 0, stream>>>(f, origin[0], origin[1], origin[2], r * r, d_paths, d_lengths, n_paths,
                                                             max_cells, max_lookahead, max_vertices, d_vertices, d_counts);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
