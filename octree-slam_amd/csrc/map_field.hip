// map_field.hip -- the distance field of a map region: for every cell of a box of cells the squared distance, in cells, to the
// nearest occupied cell of the whole root if that is within `radius_cells`, else -1 (own specification, DESIGN.md section 15: the
// reference has nothing like it; the restatement the device must equal bit for bit is tests/test_field_cpu.py).  The value is
// svoslam_pool_nearest_occupied's dist2 for a point inside the cell; it is computed for all cells at once by an exact Euclidean
// distance transform truncated at R, in integers: the occupied set is rasterised once and three separable passes follow.
//
// With the region inflated by R and clipped to the root (occupied cells up to R outside the region count):
//   field_raster_kernel  occupancy of the inflated region as bit rows, x fastest, one 64-bit word per 64 cells, the first word of
//                        a row starting at the inflated region's first x.  One lane per cell descends the tree (map_descend.hpp:
//                        section 14's descent); the 64 consecutive x of one row are one wavefront, whose ballot is the row word,
//                        written by lane 0 with one vector store.  Neighbouring lanes share all but the lowest levels of their
//                        paths, so the upper levels are cache hits.  Cells past the row's end give zero bits.
//   field_x_kernel       one lane per (x of the region, y and z of the inflated range): the distance to the nearest set bit of the
//                        row, from the row's words with count-leading / count-trailing zeros -- the own word masked below and
//                        above the cell, then whole words outwards while they can still hold something nearer -- squared if it
//                        is <= R, "none" (2^30) otherwise.
//   field_pass_kernel    the y pass (y of the region, z of the inflated range) and the z pass (writes the output): g'(i) = min
//                        over |i - j| <= R of g(j) + (i - j)^2.  One lane per column, the 64 lanes of a wavefront along x, so
//                        global accesses coalesce; one wavefront per workgroup, no barrier.  A column is cut into segments of 64
//                        outputs; a segment with its R-halo (64 + 2 R values at most, clipped to the column) is staged in LDS at
//                        dword j * 64 + lane: each lane reads back only what it wrote, 64 consecutive dwords per access, free of
//                        bank conflicts.  The search runs outwards from j = i and stops as soon as (i - j)^2 >= best, best
//                        starting at min(g(i), R^2 + 1): dense surroundings cost a few reads, and |i - j| <= R needs no test of
//                        its own.  A lane whose staged segment is all "none" (a flag kept while staging) writes "none" and is
//                        done.  A result above R^2 is "none" (-1 in the z pass): it cannot be part of a sum <= R^2.
// Which path: R <= kLdsMaxRadius (64) stages in LDS, (64 + 2 R) * 256 bytes per workgroup, 48 KB at most; a larger R runs the
// same kernel reading the intermediate from global memory (field_pass_kernel<false>): the same search, no staging.  The host
// decides from R alone.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): field_raster_kernel 18 VGPRs, field_x_kernel 16,
// field_pass_kernel<true> 13, field_pass_kernel<false> 10; every kernel 0 bytes of scratch, no static LDS, occupancy 8 by registers;
// the LDS path is bound by its dynamic LDS: 10 one-wavefront workgroups per CU at R = 0, 6 at R = 16, 3 at R = 64.  No per-lane
// arrays indexed at run time.  svoslam_pool_distance_field_profile is the same call with an event around each launch (blocking).
#include <limits.h>

#include "lattice.hpp"
#include "map_descend.hpp"
#include "map_field.hpp"
#include "stage_timing.hpp"
#include "workspace.hpp"

namespace svoslam {

namespace {

constexpr int kNone = 1 << 30;       // no set bit / no occupied cell within R so far; kNone + R^2 fits an int32
constexpr int kSeg = 64;             // outputs of one column segment
constexpr int kLdsMaxRadius = 64;    // staged rows <= kSeg + 2 * 64 = 192: 48 KB of LDS per workgroup

__global__ __launch_bounds__(256) void field_raster_kernel(const uint32_t *__restrict__ pool, int d, int x0, int y0, int z0, int x1,
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

__global__ __launch_bounds__(256) void field_x_kernel(const unsigned long long *__restrict__ bits, int wpr, int nx, int offx, int R,
                                                      long long total, int32_t *__restrict__ g) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned long long *__restrict__ w = bits + (idx / nx) * wpr;
  const int p = (int)(idx % nx) + offx, wi = p >> 6, b = p & 63;
  const unsigned long long own = w[wi];
  int best = R + 1;
  unsigned long long m = own & (~0ull >> (63 - b));  // the cell itself and below
  if (m) {
    best = min(best, b - (63 - __builtin_clzll(m)));
  } else {
    for (int k = 1; k <= wi && b + 1 + 64 * (k - 1) < best; k++) {  // the nearest a bit of word wi - k can be
      const unsigned long long v = w[wi - k];
      if (v) { best = min(best, b + 1 + 64 * (k - 1) + __builtin_clzll(v)); break; }
    }
  }
  m = own & (~0ull << b);  // the cell itself and above
  if (m) {
    best = min(best, __builtin_ctzll(m) - b);
  } else {
    for (int k = 1; wi + k < wpr && 64 - b + 64 * (k - 1) < best; k++) {
      const unsigned long long v = w[wi + k];
      if (v) { best = min(best, 64 - b + 64 * (k - 1) + __builtin_ctzll(v)); break; }
    }
  }
  g[idx] = best <= R ? best * best : kNone;
}

// in: value j of column (a, x) at in[j * stride_j + a * stride_a + x], j in [0, in_len); output i in [0, out_len) is about input
// i + off and goes to out[i * ostride_j + a * ostride_a + x].  Workgroup = (x tile, a, segment), flattened.
template <bool kLds>
__global__ __launch_bounds__(64) void field_pass_kernel(const int32_t *__restrict__ in, int nx, int xtiles, int na, int in_len,
                                                        int out_len, int off, long long stride_j, long long stride_a,
                                                        long long ostride_j, long long ostride_a, int R, int none_out,
                                                        int32_t *__restrict__ out) {
  extern __shared__ int32_t seg[];
  const int lane = threadIdx.x;
  const unsigned t = blockIdx.x / (unsigned)xtiles;
  const int x = (int)(blockIdx.x % (unsigned)xtiles) * 64 + lane, a = (int)(t % (unsigned)na), sg = (int)(t / (unsigned)na);
  if (x >= nx) return;
  const int i0 = sg * kSeg, i1 = min(i0 + kSeg, out_len);
  const int jlo = max(i0 + off - R, 0), rows = min(i1 - 1 + off + R, in_len - 1) - jlo + 1;
  const int32_t *__restrict__ col = in + (a * stride_a + x) + jlo * stride_j;
  int32_t *__restrict__ o = out + (a * ostride_a + x);
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
    int best = min(kLds ? seg[r * 64 + lane] : col[r * stride_j], cap);
    for (int k = 1; k * k < best; k++) {
      int lo = kNone, hi = kNone;
      if (r - k >= 0) lo = kLds ? seg[(r - k) * 64 + lane] : col[(r - k) * stride_j];
      if (r + k < rows) hi = kLds ? seg[(r + k) * 64 + lane] : col[(r + k) * stride_j];
      best = min(best, min(lo, hi) + k * k);
    }
    o[i * ostride_j] = best < cap ? best : none_out;
  }
}

}  // namespace

namespace {
// the profiling form's events: one before the first launch and one after each of the four
struct LaunchEvents {
  hipEvent_t ev[5] = {};
  int n = 0;
  bool on = false;
  int mark(hipStream_t stream) {
    if (!on) return SVOSLAM_OK;
    SVO_HIP(hipEventCreate(&ev[n]));
    n++;
    SVO_HIP(hipEventRecord(ev[n - 1], stream));
    return SVOSLAM_OK;
  }
  ~LaunchEvents() { for (int k = 0; k < n; k++) (void)hipEventDestroy(ev[k]); }
};
}  // namespace

int pool_distance_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                        int32_t R, int32_t *d_dist2, float *launch_ms, hipStream_t stream, long long *outer_bracket) {
  if (launch_ms) launch_ms[0] = launch_ms[1] = launch_ms[2] = launch_ms[3] = 0.0f;
  if (!ws || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_INVALID_ARG;
  if (R < 0 || R > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // R^2 + 2^30 fits an int32
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
  if (!pool || !pool->d_data || !d_dist2) return SVOSLAM_ERR_INVALID_ARG;
  const long long nx = dims[0], ny = dims[1], nz = dims[2];
  const long long wpr = (len[0] + 63) / 64, words = wpr * len[1] * len[2];
  const long long n_g1 = nx * len[1] * len[2], n_g2 = nx * ny * len[2], xtiles = (nx + 63) / 64;
  const long long segs_y = (ny + kSeg - 1) / kSeg, segs_z = (nz + kSeg - 1) / kSeg;
  const long long limit = INT_MAX;  // every side is <= 2^16, so none of these products overflows an int64
  if (nx * ny * nz > limit) {
    set_last_error_text("svoslam_pool_distance_field: %lld x %lld x %lld cells are more than 2^31 - 1", nx, ny, nz);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (words > limit || n_g1 > limit || n_g2 > limit || xtiles * len[2] * segs_y > limit || xtiles * ny * segs_z > limit) {
    set_last_error_text("svoslam_pool_distance_field: the region inflated by %d cells (%lld x %lld x %lld) needs an intermediate of "
                        "more than 2^31 - 1 elements", R, len[0], len[1], len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as extract_voxel_grid drains pending asynchronous fusions
  int rc = ws->field_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->field_a.reserve((size_t)n_g1 * 4);
  if (rc == SVOSLAM_OK) rc = ws->field_b.reserve((size_t)n_g2 * 4);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->field_bits.release(); ws->field_a.release(); ws->field_b.release();
    return rc;
  }
  unsigned long long *bits = ws->field_bits.as<unsigned long long>();
  int32_t *g1 = ws->field_a.as<int32_t>(), *g2 = ws->field_b.as<int32_t>();
  const bool lds = R <= kLdsMaxRadius;
  const size_t lds_y = lds ? (size_t)(len[1] < kSeg + 2 * R ? len[1] : kSeg + 2 * R) * 256 : 0;
  const size_t lds_z = lds ? (size_t)(len[2] < kSeg + 2 * R ? len[2] : kSeg + 2 * R) * 256 : 0;
  const int off_x = (int)(origin[0] - lo[0]), off_y = (int)(origin[1] - lo[1]), off_z = (int)(origin[2] - lo[2]);
  LaunchEvents timed;
  timed.on = launch_ms != nullptr;
  // a caller that goes on after the field (map_reach.hip) owns the bracket: it is opened here, where nothing can be refused any
  // more, and closed by the caller
  if (outer_bracket) (void)stage_begin(kStageQuery, stream, outer_bracket);
  StageScope query(outer_bracket ? -1 : (int)kStageQuery, stream);
  SVO_TRY(timed.mark(stream));
  field_raster_kernel<<<cdiv(words, 4), 256, 0, stream>>>(pool->d_data, depth, (int)lo[0], (int)lo[1], (int)lo[2], (int)(lo[0] + len[0]),
                                                          (int)wpr, (int)len[1], words, bits);
  SVO_LAUNCH_CHECK();
  SVO_TRY(timed.mark(stream));
  field_x_kernel<<<cdiv(n_g1, 256), 256, 0, stream>>>(bits, (int)wpr, (int)nx, off_x, R, n_g1, g1);
  SVO_LAUNCH_CHECK();
  SVO_TRY(timed.mark(stream));
  // y: columns (z of the inflated range, x), g1[z][y'][x] -> g2[z][y][x]
  const unsigned blocks_y = (unsigned)(xtiles * len[2] * segs_y), blocks_z = (unsigned)(xtiles * ny * segs_z);
  if (lds)
    field_pass_kernel<true><<<blocks_y, 64, lds_y, stream>>>(g1, (int)nx, (int)xtiles, (int)len[2], (int)len[1], (int)ny, off_y, nx,
                                                             len[1] * nx, nx, ny * nx, R, kNone, g2);
  else
    field_pass_kernel<false><<<blocks_y, 64, 0, stream>>>(g1, (int)nx, (int)xtiles, (int)len[2], (int)len[1], (int)ny, off_y, nx,
                                                          len[1] * nx, nx, ny * nx, R, kNone, g2);
  SVO_LAUNCH_CHECK();
  SVO_TRY(timed.mark(stream));
  // z: columns (y, x), g2[z'][y][x] -> dist2[z][y][x]
  if (lds)
    field_pass_kernel<true><<<blocks_z, 64, lds_z, stream>>>(g2, (int)nx, (int)xtiles, (int)ny, (int)len[2], (int)nz, off_z, ny * nx, nx,
                                                             ny * nx, nx, R, -1, d_dist2);
  else
    field_pass_kernel<false><<<blocks_z, 64, 0, stream>>>(g2, (int)nx, (int)xtiles, (int)ny, (int)len[2], (int)nz, off_z, ny * nx, nx,
                                                          ny * nx, nx, R, -1, d_dist2);
  SVO_LAUNCH_CHECK();
  if (launch_ms) {  // the profiling form blocks
    SVO_TRY(timed.mark(stream));
    SVO_HIP(hipEventSynchronize(timed.ev[4]));
    for (int k = 0; k < 4; k++) SVO_HIP(hipEventElapsedTime(&launch_ms[k], timed.ev[k], timed.ev[k + 1]));
  }
  return SVOSLAM_OK;
}

// section 14's "Box to cells" on the host: the planes, the counts and the emptiness test of count_boxes_kernel (lattice.hpp)
int box_to_cells(int depth, const float center[3], float edge, const float box[6], int32_t lo[3], int32_t hi[3], int32_t *empty) {
  if (depth < 1 || depth > SVOSLAM_MAX_DEPTH || !center || !(edge > 0.0f) || !box || !lo || !hi || !empty) return SVOSLAM_ERR_INVALID_ARG;
  const int N = 1 << depth;
  const float h = edge / (float)N;
  bool none = false;
  for (int a = 0; a < 3; a++) {
    const float mn = box[a], mx = box[3 + a];
    if (!(mn <= mx) || mx < lattice_plane(center[a], 0, N, h) || mn > lattice_plane(center[a], N, N, h)) none = true;  // a NaN: !(mn <= mx)
    lo[a] = cell_in_block(center[a], N, h, mn, 0, N, false);
    const int k = cell_in_block(center[a], N, h, mx, 0, N, true);
    hi[a] = k > lo[a] ? k : lo[a];
  }
  *empty = none ? 1 : 0;
  return SVOSLAM_OK;
}

}  // namespace svoslam
