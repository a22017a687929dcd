// map_visibility.hip -- the visibility field of a map region: for every cell q of a box of cells the viewpoints v with
// |q - v|^2 <= R^2 whose line of sight to q is free -- no occupied cell, other than v and q themselves, whose closed cube meets the
// closed segment between the two cell centres (the supercover of the segment without its ends; own specification, DESIGN.md section
// 19; the restatement the device must equal bit for bit is tests/test_visibility_cpu.py).  Pure integers, symmetric in v and q.
//
// With the region inflated by R and clipped to the root (every cell between a counting viewpoint within range and its target lies
// in it, because it lies in their bounding box):
//   vis_raster_kernel   field_raster_kernel a third time: one wavefront per 64-bit row word, one descent per cell, a ballot.  An
//                       instantiation of this file's own, so that map_field.hip's and map_nearest.hip's generated code stay as they
//                       are; folding the three copies into one is a refactor of its own.
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
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): vis_raster_kernel 18 VGPRs / 31 SGPRs, sight_kernel 42 VGPRs / 62 SGPRs;
// both 0 bytes of scratch, no LDS.  No per-lane arrays; every store is a vector store from plain C++.
#include <limits.h>

#include "map_descend.hpp"
#include "map_visibility.hpp"
#include "stage_timing.hpp"
#include "workspace.hpp"

namespace svoslam {

namespace {

constexpr long long kNever = 1ll << 62;  // the key of an axis along which the segment does not move

__global__ __launch_bounds__(256) void vis_raster_kernel(const uint32_t *__restrict__ pool, int d, int x0, int y0, int z0, int x1,
                                                         int wpr, int iny, long long words, unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const long long row = word / wpr;
  const int x = x0 + (int)(word % wpr) * 64 + lane, y = y0 + (int)(row % iny), z = z0 + (int)(row / iny);
  bool hit = false;
  if (x < x1) {
    uint32_t nd = 0u;
    uint2 w = make_uint2(0u, 0u);
    descend<false>(pool, morton3(x, y, z), d, x, y, z, 0, 0, 0, 0, nd, w, hit);
  }
  const unsigned long long row_word = __ballot(hit);
  if (lane == 0) bits[word] = row_word;
}

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
  if (!ws || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_INVALID_ARG;
  if (R < 0 || R > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // 3 R^2 fits an int32, a key fits an int64
  if (n_views < 0 || (n_views > 0 && !d_views)) return SVOSLAM_ERR_INVALID_ARG;
  if (d_mask && n_views > SVOSLAM_MAX_VIEWS_MASK) return SVOSLAM_ERR_INVALID_ARG;  // a bit per viewpoint
  const long long N = 1ll << depth;
  long long lo[3], len[3];  // the inflated region: first cell and cells per axis
  bool nothing = false;
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > N) return SVOSLAM_ERR_INVALID_ARG;
    nothing = nothing || dims[a] == 0;
    lo[a] = origin[a] - R > 0 ? origin[a] - R : 0;
    const long long end = (long long)origin[a] + dims[a] + R < N ? (long long)origin[a] + dims[a] + R : N;
    len[a] = end - lo[a];
  }
  if (nothing) return SVOSLAM_OK;
  if (!pool || !pool->d_data || (!d_mask && !d_count)) return SVOSLAM_ERR_INVALID_ARG;
  const long long nx = dims[0], ny = dims[1], nz = dims[2];
  const long long wpr = (len[0] + 63) / 64, words = wpr * len[1] * len[2], n_out = nx * ny * nz;
  const long long limit = INT_MAX;  // every side is <= 2^16, so neither product overflows an int64
  if (n_out > limit) {
    set_last_error_text("svoslam_pool_visibility_field: %lld x %lld x %lld cells are more than 2^31 - 1", nx, ny, nz);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (words > limit) {
    set_last_error_text("svoslam_pool_visibility_field: the region inflated by %d cells (%lld x %lld x %lld) needs more than 2^31 - 1 "
                        "row words", R, len[0], len[1], len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as pool_distance_field drains pending asynchronous fusions
  const int rc = ws->vis_bits.reserve((size_t)words * 8);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->vis_bits.release();
    return rc;
  }
  unsigned long long *bits = ws->vis_bits.as<unsigned long long>();
  StageScope query(kStageQuery, stream);
  vis_raster_kernel<<<cdiv(words, 4), 256, 0, stream>>>(pool->d_data, depth, (int)lo[0], (int)lo[1], (int)lo[2], (int)(lo[0] + len[0]),
                                                        (int)wpr, (int)len[1], words, bits);
  SVO_LAUNCH_CHECK();
  sight_kernel<<<cdiv(n_out, 256), 256, 0, stream>>>(bits, (int)wpr, (int)len[1], (int)lo[0], (int)lo[1], (int)lo[2], origin[0],
                                                     origin[1], origin[2], (int)nx, (int)ny, (int)N, R, d_views, n_views, (int)n_out,
                                                     d_mask, d_count);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
