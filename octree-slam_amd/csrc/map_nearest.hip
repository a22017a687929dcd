// map_nearest.hip -- the nearest-cell field of a map region: for every cell of a box of cells the squared distance, in cells, to the
// nearest cell of a target set A within `radius_cells` AND that cell, the witness: the one with the smallest z, then y, then x among
// the equally near (own specification; the restatement the device must equal bit for bit is
// tests/test_nearest_cpu.py).  A is the occupied cells of the root (then the witness's node and colour word can be had too) or the
// cells of the root that are not occupied.  The route is map_field.hip's exact truncated distance transform, whose three passes
// each also keep WHERE their minimum lies; the kernels are copies of map_field.hip's with that added, so the distance field's own
// kernels and their generated code are untouched.
//
// With the region inflated by R and clipped to the root (target cells up to R outside the region count):
//   nearest_raster_kernel   field_raster_kernel, with the bit of a cell that is in the row and NOT occupied set instead when the free
//                           cells are asked for.  The test x < x1 comes before the inversion, so the lanes past the row's end give
//                           zero bits in both forms; x1 <= N, so nothing outside the root is ever a cell.
//   nearest_x_kernel        field_x_kernel's search of the row words, below and above the cell.  The side below is taken first and
//                           the side above only if it is strictly nearer: on a tie the smaller x wins.  Writes g1 and the witness's
//                           x (as an index into the inflated row, 16 bits).
//   nearest_pass_kernel     field_pass_kernel's staging and outward search for g'(i) = min over j of g(j) + (i - j)^2, which also
//                           writes the SMALLEST j that attains the minimum.  The search visits k while k^2 <= best, one step more
//                           than the minimum alone needs: a row at j = i - k with g = 0 and k^2 == best ties with the best so far
//                           and, being lower, wins.  At step k everything seen so far lies in (i - k, i + k), so the low candidate
//                           takes the place on `<=` and the high one only on `<`; the low one is compared first, so that on equal
//                           sums at the same k the low one stays.  The argmin lives in a register: the LDS budget is the distance
//                           field's, (64 + 2 R) * 256 bytes, with the same switch to the global-memory form above R = 64.
//   nearest_resolve_kernel  one lane per output cell follows the three indices: z' from the z pass, y' = the y pass's argmin at
//                           (x, y, z'), x' = the x pass's witness at (x, y', z'); only one 16-bit index per pass is ever stored.
//                           With node / colour asked for, one descent (map_descend.hpp) to (x', y', z') follows; neighbouring lanes
//                           mostly share the witness.  It writes dist2, cell, node and colour, each only if asked for.
// An index is only followed from a value that is not "none", and such a value is a sum whose terms are not "none" either, so
// every index that is read was written (DESIGN.md section 18 has the argument for the tie rule).
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): nearest_raster_kernel 18 VGPRs, nearest_x_kernel 17,
// nearest_pass_kernel<true> 18, nearest_pass_kernel<false> 14, nearest_resolve_kernel<true> (node / colour) 15, <false> 11; every
// kernel 0 bytes of scratch, no static LDS, occupancy 8 by registers; the LDS path is bound by its dynamic LDS exactly as
// field_pass_kernel is (10 one-wavefront workgroups per CU at R = 0, 6 at R = 16, 3 at R = 64).  No per-lane arrays indexed at run
// time; every store is a vector store from plain C++.
#include <limits.h>

#include "map_descend.hpp"
#include "map_nearest.hpp"
#include "stage_timing.hpp"
#include "workspace.hpp"

namespace svoslam {

namespace {

constexpr int kNone = 1 << 30;       // no set bit / no target cell within R so far; kNone + R^2 fits an int32
constexpr int kSeg = 64;             // outputs of one column segment
constexpr int kLdsMaxRadius = 64;    // staged rows <= kSeg + 2 * 64 = 192: 48 KB of LDS per workgroup

__global__ __launch_bounds__(256) void nearest_raster_kernel(const uint32_t *__restrict__ pool, int d, int x0, int y0, int z0, int x1,
                                                             int wpr, int iny, long long words, bool free_cells,
                                                             unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const long long row = word / wpr;
  const int x = x0 + (int)(word % wpr) * 64 + lane, y = y0 + (int)(row % iny), z = z0 + (int)(row / iny);
  bool target = false;
  if (x < x1) {
    uint32_t nd = 0u;
    uint2 w = make_uint2(0u, 0u);
    bool hit = false;
    descend<false>(pool, morton3(x, y, z), d, x, y, z, 0, 0, 0, 0, nd, w, hit);
    target = hit != free_cells;
  }
  const unsigned long long row_word = __ballot(target);
  if (lane == 0) bits[word] = row_word;
}

__global__ __launch_bounds__(256) void nearest_x_kernel(const unsigned long long *__restrict__ bits, int wpr, int nx, int offx, int R,
                                                        long long total, int32_t *__restrict__ g, uint16_t *__restrict__ wit) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned long long *__restrict__ w = bits + (idx / nx) * wpr;
  const int p = (int)(idx % nx) + offx, wi = p >> 6, b = p & 63;
  const unsigned long long own = w[wi];
  int best = R + 1, at = p;
  unsigned long long m = own & (~0ull >> (63 - b));  // the cell itself and below
  if (m) {
    const int dist = b - (63 - __builtin_clzll(m));
    if (dist < best) { best = dist; at = p - dist; }
  } else {
    for (int k = 1; k <= wi && b + 1 + 64 * (k - 1) < best; k++) {  // the nearest a bit of word wi - k can be
      const unsigned long long v = w[wi - k];
      if (v) {
        const int dist = b + 1 + 64 * (k - 1) + __builtin_clzll(v);
        if (dist < best) { best = dist; at = p - dist; }
        break;
      }
    }
  }
  m = own & (~0ull << b);  // the cell itself and above: only what is strictly nearer than the side below
  if (m) {
    const int dist = __builtin_ctzll(m) - b;
    if (dist < best) { best = dist; at = p + dist; }
  } else {
    for (int k = 1; wi + k < wpr && 64 - b + 64 * (k - 1) < best; k++) {
      const unsigned long long v = w[wi + k];
      if (v) {
        const int dist = 64 - b + 64 * (k - 1) + __builtin_ctzll(v);
        if (dist < best) { best = dist; at = p + dist; }
        break;
      }
    }
  }
  g[idx] = best <= R ? best * best : kNone;
  wit[idx] = (uint16_t)at;
}

// in: value j of column (a, x) at in[j * stride_j + a * stride_a + x], j in [0, in_len); output i in [0, out_len) is about input
// i + off and goes to out[i * ostride_j + a * ostride_a + x], the smallest j of its minimum to arg[the same index].  Workgroup =
// (x tile, a, segment), flattened.
template <bool kLds>
__global__ __launch_bounds__(64) void nearest_pass_kernel(const int32_t *__restrict__ in, int nx, int xtiles, int na, int in_len,
                                                          int out_len, int off, long long stride_j, long long stride_a,
                                                          long long ostride_j, long long ostride_a, int R, int none_out,
                                                          int32_t *__restrict__ out, uint16_t *__restrict__ arg) {
  extern __shared__ int32_t seg[];
  const int lane = threadIdx.x;
  const unsigned t = blockIdx.x / (unsigned)xtiles;
  const int x = (int)(blockIdx.x % (unsigned)xtiles) * 64 + lane, a = (int)(t % (unsigned)na), sg = (int)(t / (unsigned)na);
  if (x >= nx) return;
  const int i0 = sg * kSeg, i1 = min(i0 + kSeg, out_len);
  const int jlo = max(i0 + off - R, 0), rows = min(i1 - 1 + off + R, in_len - 1) - jlo + 1;
  const int32_t *__restrict__ col = in + (a * stride_a + x) + jlo * stride_j;
  int32_t *__restrict__ o = out + (a * ostride_a + x);
  uint16_t *__restrict__ oa = arg + (a * ostride_a + x);
  if (kLds) {
    bool any = false;
    for (int r = 0; r < rows; r++) {
      const int v = col[r * stride_j];
      seg[r * 64 + lane] = v;
      any = any || v != kNone;
    }
    if (!any) {
      for (int i = i0; i < i1; i++) o[i * ostride_j] = none_out;
      return;
    }
  }
  const int cap = R * R + 1;
  for (int i = i0; i < i1; i++) {
    const int r = i + off - jlo;
    int best = min(kLds ? seg[r * 64 + lane] : col[r * stride_j], cap), at = r;
    for (int k = 1; k * k <= best; k++) {
      int lo = kNone, hi = kNone;
      if (r - k >= 0) lo = kLds ? seg[(r - k) * 64 + lane] : col[(r - k) * stride_j];
      if (r + k < rows) hi = kLds ? seg[(r + k) * 64 + lane] : col[(r + k) * stride_j];
      lo += k * k;
      hi += k * k;
      if (lo <= best) { best = lo; at = r - k; }
      if (hi < best) { best = hi; at = r + k; }
    }
    o[i * ostride_j] = best < cap ? best : none_out;
    oa[i * ostride_j] = (uint16_t)(jlo + at);
  }
}

// g3, az: the z pass's output [nz][ny][nx]; ay: the y pass's argmin [len z][ny][nx]; wx: the x pass's witness [len z][len y][nx]
template <bool kNode>
__global__ __launch_bounds__(256) void nearest_resolve_kernel(const uint32_t *__restrict__ pool, int d, const int32_t *__restrict__ g3,
                                                              const uint16_t *__restrict__ az, const uint16_t *__restrict__ ay,
                                                              const uint16_t *__restrict__ wx, int nx, int ny, int leny, int lox,
                                                              int loy, int loz, int total, int32_t *__restrict__ out_dist2,
                                                              unsigned long long *__restrict__ out_cell,
                                                              int32_t *__restrict__ out_node, uint32_t *__restrict__ out_color) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  if (lane_idx >= (unsigned)total) return;
  const int idx = (int)lane_idx;
  const int dist2 = g3[idx];
  unsigned long long cell = ~0ull;
  int32_t node = -1;
  uint32_t color = 0u;
  if (dist2 >= 0) {
    const int x = idx % nx, y = (idx / nx) % ny;
    const long long zr = az[idx];
    const long long yr = ay[(zr * ny + y) * nx + x];
    const int xr = wx[(zr * leny + yr) * nx + x];
    const int cx = lox + xr, cy = loy + (int)yr, cz = loz + (int)zr;
    cell = (unsigned long long)cx | ((unsigned long long)cy << 16) | ((unsigned long long)cz << 32);
    if (kNode) {
      uint32_t nd = 0u;
      uint2 w = make_uint2(0u, 0u);
      bool hit = false;
      descend<false>(pool, morton3(cx, cy, cz), d, cx, cy, cz, 0, 0, 0, 0, nd, w, hit);
      if (hit) { node = (int32_t)nd; color = w.y; }
    }
  }
  if (out_dist2) out_dist2[idx] = dist2;
  if (out_cell) out_cell[idx] = cell;
  if (kNode) {
    if (out_node) out_node[idx] = node;
    if (out_color) out_color[idx] = color;
  }
}

}  // namespace

int pool_nearest_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                       int32_t R, int32_t which, int32_t *d_dist2, uint64_t *d_cell, int32_t *d_node, uint32_t *d_color,
                       hipStream_t stream) {
  if (!ws || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_INVALID_ARG;
  if (R < 0 || R > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // R^2 + 2^30 fits an int32
  if (which != SVOSLAM_NEAREST_OCCUPIED && which != SVOSLAM_NEAREST_FREE) return SVOSLAM_ERR_INVALID_ARG;
  if (which == SVOSLAM_NEAREST_FREE && (d_node || d_color)) return SVOSLAM_ERR_INVALID_ARG;  // a free cell has no level-d node
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
  if (!pool || !pool->d_data || (!d_dist2 && !d_cell && !d_node && !d_color)) return SVOSLAM_ERR_INVALID_ARG;
  const long long nx = dims[0], ny = dims[1], nz = dims[2];
  const long long wpr = (len[0] + 63) / 64, words = wpr * len[1] * len[2];
  const long long n_g1 = nx * len[1] * len[2], n_g2 = nx * ny * len[2], n_out = nx * ny * nz, xtiles = (nx + 63) / 64;
  const long long segs_y = (ny + kSeg - 1) / kSeg, segs_z = (nz + kSeg - 1) / kSeg;
  const long long limit = INT_MAX;  // every side is <= 2^16, so none of these products overflows an int64
  if (n_out > limit) {
    set_last_error_text("svoslam_pool_nearest_field: %lld x %lld x %lld cells are more than 2^31 - 1", nx, ny, nz);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (words > limit || n_g1 > limit || n_g2 > limit || xtiles * len[2] * segs_y > limit || xtiles * ny * segs_z > limit) {
    set_last_error_text("svoslam_pool_nearest_field: the region inflated by %d cells (%lld x %lld x %lld) needs an intermediate of "
                        "more than 2^31 - 1 elements", R, len[0], len[1], len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as pool_distance_field drains pending asynchronous fusions
  // one slot for the bit rows, one for the three value arrays (after the x, the y and the z pass), one for their three indices
  int rc = ws->near_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->near_dist.reserve((size_t)(n_g1 + n_g2 + n_out) * 4);
  if (rc == SVOSLAM_OK) rc = ws->near_arg.reserve((size_t)(n_g1 + n_g2 + n_out) * 2);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->near_bits.release(); ws->near_dist.release(); ws->near_arg.release();
    return rc;
  }
  unsigned long long *bits = ws->near_bits.as<unsigned long long>();
  int32_t *g1 = ws->near_dist.as<int32_t>(), *g2 = g1 + n_g1, *g3 = g2 + n_g2;
  uint16_t *wx = ws->near_arg.as<uint16_t>(), *ay = wx + n_g1, *az = ay + n_g2;
  const bool lds = R <= kLdsMaxRadius;
  const size_t lds_y = lds ? (size_t)(len[1] < kSeg + 2 * R ? len[1] : kSeg + 2 * R) * 256 : 0;
  const size_t lds_z = lds ? (size_t)(len[2] < kSeg + 2 * R ? len[2] : kSeg + 2 * R) * 256 : 0;
  const int off_x = (int)(origin[0] - lo[0]), off_y = (int)(origin[1] - lo[1]), off_z = (int)(origin[2] - lo[2]);
  StageScope query(kStageQuery, stream);
  nearest_raster_kernel<<<cdiv(words, 4), 256, 0, stream>>>(pool->d_data, depth, (int)lo[0], (int)lo[1], (int)lo[2], (int)(lo[0] + len[0]),
                                                            (int)wpr, (int)len[1], words, which == SVOSLAM_NEAREST_FREE, bits);
  SVO_LAUNCH_CHECK();
  nearest_x_kernel<<<cdiv(n_g1, 256), 256, 0, stream>>>(bits, (int)wpr, (int)nx, off_x, R, n_g1, g1, wx);
  SVO_LAUNCH_CHECK();
  // y: columns (z of the inflated range, x), g1[z'][y'][x] -> g2[z'][y][x]
  const unsigned blocks_y = (unsigned)(xtiles * len[2] * segs_y), blocks_z = (unsigned)(xtiles * ny * segs_z);
  if (lds)
    nearest_pass_kernel<true><<<blocks_y, 64, lds_y, stream>>>(g1, (int)nx, (int)xtiles, (int)len[2], (int)len[1], (int)ny, off_y, nx,
                                                               len[1] * nx, nx, ny * nx, R, kNone, g2, ay);
  else
    nearest_pass_kernel<false><<<blocks_y, 64, 0, stream>>>(g1, (int)nx, (int)xtiles, (int)len[2], (int)len[1], (int)ny, off_y, nx,
                                                            len[1] * nx, nx, ny * nx, R, kNone, g2, ay);
  SVO_LAUNCH_CHECK();
  // z: columns (y, x), g2[z'][y][x] -> g3[z][y][x]
  if (lds)
    nearest_pass_kernel<true><<<blocks_z, 64, lds_z, stream>>>(g2, (int)nx, (int)xtiles, (int)ny, (int)len[2], (int)nz, off_z, ny * nx, nx,
                                                               ny * nx, nx, R, -1, g3, az);
  else
    nearest_pass_kernel<false><<<blocks_z, 64, 0, stream>>>(g2, (int)nx, (int)xtiles, (int)ny, (int)len[2], (int)nz, off_z, ny * nx, nx,
                                                            ny * nx, nx, R, -1, g3, az);
  SVO_LAUNCH_CHECK();
  unsigned long long *cell = reinterpret_cast<unsigned long long *>(d_cell);
  if (d_node || d_color)
    nearest_resolve_kernel<true><<<cdiv(n_out, 256), 256, 0, stream>>>(pool->d_data, depth, g3, az, ay, wx, (int)nx, (int)ny, (int)len[1],
                                                                       (int)lo[0], (int)lo[1], (int)lo[2], (int)n_out, d_dist2, cell,
                                                                       d_node, d_color);
  else
    nearest_resolve_kernel<false><<<cdiv(n_out, 256), 256, 0, stream>>>(pool->d_data, depth, g3, az, ay, wx, (int)nx, (int)ny, (int)len[1],
                                                                        (int)lo[0], (int)lo[1], (int)lo[2], (int)n_out, d_dist2, cell,
                                                                        d_node, d_color);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
