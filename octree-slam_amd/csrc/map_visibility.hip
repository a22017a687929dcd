// map_visibility.hip -- the visibility field of a map region: for every cell q of a box of cells the viewpoints v with
// |q - v|^2 <= R^2 whose line of sight to q is free -- no occupied cell, other than v and q themselves, whose closed cube meets the
// closed segment between the two cell centres (the supercover of the segment without its ends; own specification, DESIGN.md section
// 19; the restatement the device must equal bit for bit is tests/test_visibility_cpu.py).  Pure integers, symmetric in v and q.
//
// With the region inflated by R and clipped to the root (every cell between a counting viewpoint within range and its target lies
// in it, because it lies in their bounding box):
//   the raster          map_region.hip's region_raster_kernel, as the distance field runs it: the occupied cells as 64-bit row words.
//   sight_kernel        one lane per output cell, x fastest.  The loop over the viewpoints is uniform across the wavefront and the
//                       viewpoint is read through a uniform index.  Per viewpoint the range test, then the walk from v towards q.
//                       With D = q - v the segment crosses axis a's i-th face at (2 i - 1) / (2 |D_a|); the kernel keeps per axis
//                       the key (2 i_a + 1) * (the product of the other two |D|, a zero taken as 1), which orders the next
//                       crossings exactly as cross-multiplication does, grows by a constant per step and stays below 2^38.  An axis
//                       with D_a = 0 never crosses (key 2^62); an axis that has made all its crossings has a key above every live
//                       one (its parameter would be above 1), so it needs no flag.  Equal keys are a tie: the segment passes through
//                       an edge or a corner, and the 2 or 6 side cells are tested before the diagonal step.  v is never tested; the
//                       walk stops on entering q without testing it, after the side cells of a tie that ends there; it leaves at
//                       the first set bit.  Neighbouring lanes share v and end next to each other, so their first steps read the
//                       same row words.  The three keys, their increments and the current cell are named scalars.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): sight_kernel 42 VGPRs / 62 SGPRs, 0 bytes of scratch, no
// LDS.  No per-lane arrays; every store is a vector store from plain C++.
#include "map_region.hpp"
#include "map_visibility.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr long long kNever = 1ll << 62;  // the key of an axis along which the segment does not move

// the bit of cell (x, y, z) of the inflated region (coordinates relative to its first cell)
__device__ __forceinline__ bool occupied(const unsigned long long *__restrict__ bits, int wpr, int leny, int x, int y, int z) {
  return (bits[((long long)z * leny + y) * wpr + (x >> 6)] >> (x & 63)) & 1ull;
}

// (lox, loy, loz), leny, wpr: the inflated region's first cell, rows per plane and words per row; (ox, oy, oz), nx, ny: the region
__global__ __launch_bounds__(256) void sight_kernel(const unsigned long long *__restrict__ bits, int wpr, int leny, int lox, int loy,
                                                    int loz, int ox, int oy, int oz, int nx, int ny, int n_side, int R,
                                                    const int32_t *__restrict__ views, int n_views, int total,
                                                    uint32_t *__restrict__ out_mask, int32_t *__restrict__ out_count) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  if (lane_idx >= (unsigned)total) return;
  const int idx = (int)lane_idx;
  const int qx = ox + idx % nx, qy = oy + (idx / nx) % ny, qz = oz + idx / nx / ny;
  const int R2 = R * R;
  uint32_t mask = 0u;
  int count = 0;
  for (int k = 0; k < n_views; k++) {
    const int vx = views[3 * k], vy = views[3 * k + 1], vz = views[3 * k + 2];
    if ((unsigned)vx >= (unsigned)n_side || (unsigned)vy >= (unsigned)n_side || (unsigned)vz >= (unsigned)n_side) continue;
    const int dx = qx - vx, dy = qy - vy, dz = qz - vz;
    const int ax = abs(dx), ay = abs(dy), az = abs(dz);
    if (ax > R || ay > R || az > R) continue;  // each term below is then at most 4096^2
    if (ax * ax + ay * ay + az * az > R2) continue;
    bool seen = true;
    if (ax | ay | az) {
      const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1, sz = dz < 0 ? -1 : 1;
      const long long mx = max(ax, 1), my = max(ay, 1), mz = max(az, 1);
      const long long gx = 2 * my * mz, gy = 2 * mx * mz, gz = 2 * mx * my;  // what a key grows by per crossing
      long long kx = ax ? my * mz : kNever, ky = ay ? mx * mz : kNever, kz = az ? mx * my : kNever;
      int cx = vx - lox, cy = vy - loy, cz = vz - loz;
      const int tx = qx - lox, ty = qy - loy, tz = qz - loz;
      for (;;) {
        const long long first = min(kx, min(ky, kz));
        const bool bx = kx == first, by = ky == first, bz = kz == first;
        const int ex = bx ? sx : 0, ey = by ? sy : 0, ez = bz ? sz : 0;
        if ((int)bx + (int)by + (int)bz > 1) {  // through an edge or a corner: the cells beside the diagonal step
          bool hit = false;
          if (bx) hit = occupied(bits, wpr, leny, cx + ex, cy, cz);
          if (by) hit = hit || occupied(bits, wpr, leny, cx, cy + ey, cz);
          if (bz) hit = hit || occupied(bits, wpr, leny, cx, cy, cz + ez);
          if (bx && by && bz)
            hit = hit || occupied(bits, wpr, leny, cx + ex, cy + ey, cz) || occupied(bits, wpr, leny, cx + ex, cy, cz + ez) ||
                  occupied(bits, wpr, leny, cx, cy + ey, cz + ez);
          if (hit) { seen = false; break; }
        }
        cx += ex; cy += ey; cz += ez;
        if (bx) kx += gx;
        if (by) ky += gy;
        if (bz) kz += gz;
        if (cx == tx && cy == ty && cz == tz) break;
        if (occupied(bits, wpr, leny, cx, cy, cz)) { seen = false; break; }
      }
    }
    if (seen) {
      if (k < SVOSLAM_MAX_VIEWS_MASK) mask |= 1u << k;
      count++;
    }
  }
  if (out_mask) out_mask[idx] = mask;
  if (out_count) out_count[idx] = count;
}

}  // namespace

int pool_visibility_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                          int32_t R, const int32_t *d_views, int32_t n_views, uint32_t *d_mask, int32_t *d_count, hipStream_t stream) {
  if (!ws || n_views < 0 || (n_views > 0 && !d_views)) return SVOSLAM_ERR_INVALID_ARG;
  if (d_mask && n_views > SVOSLAM_MAX_VIEWS_MASK) return SVOSLAM_ERR_INVALID_ARG;  // a bit per viewpoint
  RegionPlan p;  // R <= SVOSLAM_MAX_RADIUS_CELLS: 3 R^2 fits an int32, a key fits an int64
  SVO_TRY(plan_region(depth, origin, dims, R, &p));
  if (p.nothing) return SVOSLAM_OK;
  if (!d_mask && !d_count) return SVOSLAM_ERR_INVALID_ARG;
  SVO_TRY(admit_region("svoslam_pool_visibility_field", pool, p, R, false, stream));
  const int rc = ws->vis_bits.reserve((size_t)p.words * 8);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->vis_bits.release();
    return rc;
  }
  unsigned long long *bits = ws->vis_bits.as<unsigned long long>();
  StageScope query(kStageQuery, stream);
  SVO_TRY(region_raster(pool, depth, p, false, bits, stream));
  sight_kernel<<<cdiv(p.n_out, 256), 256, 0, stream>>>(bits, (int)p.wpr, (int)p.len[1], (int)p.lo[0], (int)p.lo[1], (int)p.lo[2],
                                                       origin[0], origin[1], origin[2], (int)p.nx, (int)p.ny, 1 << depth, R, d_views,
                                                       n_views, (int)p.n_out, d_mask, d_count);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
