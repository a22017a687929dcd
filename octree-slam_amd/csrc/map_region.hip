// map_region.hip -- the inflated region of the map's region fields, its raster and its distance transform, each written once
// (DESIGN.md section 15).  The distance field (map_field.hip), the nearest-cell field (map_nearest.hip) and the visibility field
// (map_visibility.hip) plan, admit and rasterise here; the first two transform here; the reach field (map_reach.hip) and the
// component labels (map_components.hip) plan their own region with R = 0 and pack the field's -1 into its bit rows here.
//
// With the region inflated by R and clipped to the root (cells up to R outside the region count):
//   region_raster_kernel  the inflated region as bit rows, x fastest, one 64-bit word per 64 cells, the first word of a row starting
//                         at the inflated region's first x.  One lane per cell descends the tree (map_descend.hpp: section 14's
//                         descent); the 64 consecutive x of one row are one wavefront, whose ballot is the row word, written by
//                         lane 0 with one vector store.  Neighbouring lanes share all but the lowest levels of their paths, so the
//                         upper levels are cache hits.  The bit is "occupied", or with `complement` "a cell of the row that is not
//                         occupied": the test x < x1 comes before the inversion, so the lanes past the row's end give zero bits
//                         in both forms; x1 <= N, so nothing outside the root is ever a cell.
//   edt_x_kernel<kArg>    one lane per (x of the region, y and z of the inflated range): the distance to the nearest set bit of the
//                         row, from the row's words with count-leading / count-trailing zeros -- the own word masked below and
//                         above the cell, then whole words outwards while they can still hold something nearer -- squared if it
//                         is <= R, "none" (2^30) otherwise.  The side below is taken first and the side above only if it is
//                         strictly nearer; kArg also writes the bit's x (an index into the inflated row, 16 bits): on a tie the
//                         smaller x.
//   edt_pass_kernel<kLds, kArg>
//                         the y pass (y of the region, z of the inflated range) and the z pass (writes the output): g'(i) = min
//                         over |i - j| <= R of g(j) + (i - j)^2.  One lane per column, the 64 lanes of a wavefront along x, so
//                         global accesses coalesce; one wavefront per workgroup, no barrier.  A column is cut into segments of 64
//                         outputs; a segment with its R-halo (64 + 2 R values at most, clipped to the column) is staged in LDS at
//                         dword j * 64 + lane: each lane reads back only what it wrote, 64 consecutive dwords per access, free of
//                         bank conflicts.  The search runs outwards from j = i and stops as soon as (i - j)^2 >= best, best
//                         starting at min(g(i), R^2 + 1): dense surroundings cost a few reads, and |i - j| <= R needs no test of
//                         its own.  A lane whose staged segment is all "none" (a flag kept while staging) writes "none" and is
//                         done.  A result above R^2 is "none" (-1 in the z pass): it cannot be part of a sum <= R^2.
//                         kArg also writes the SMALLEST j that attains the minimum.  Its search visits k while k^2 <= best, one
//                         step more than the minimum alone needs: a row at j = i - k with g = 0 and k^2 == best ties with the best
//                         so far and, being lower, wins.  At step k everything seen so far lies in (i - k, i + k), so the low
//                         candidate takes the place on `<=` and the high one only on `<`; the low one is compared first, so that on
//                         equal sums at the same k the low one stays.  The argmin lives in a register.
//   region_pack_kernel<kOverwrite>
//                         one wavefront per 64 consecutive x of a row of the region itself: the ballot of (value == -1) != invert
//                         is the row word (the raster's layout), written by lane 0 with one vector store; kOverwrite: every lane
//                         then overwrites its own value with the caller's "none", so the array becomes a working array in place.
// The ground field (map_ground.hip, section 23) plans with an inflation per axis and side (plan_region_axes) and transforms within
// the layers of its up axis only (region_transform_planar): edt_x_kernel<false> and one edt_pass_kernel along the other horizontal
// axis, the same kernels launched with that axis' strides; the pass along up is left out.
// Which path: R <= kLdsMaxRadius (64) stages in LDS, (64 + 2 R) * 256 bytes per workgroup, 48 KB at most; a larger R runs the
// same kernel reading the intermediate from global memory (kLds = false): the same search, no staging.  The host decides from R
// alone.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): region_raster_kernel 18 VGPRs; edt_x_kernel<false> 16,
// <true> 17; edt_pass_kernel<true, false> 13, <false, false> 10, <true, true> 18, <false, true> 14; region_pack_kernel 14; every
// kernel 0 bytes of scratch, no static LDS, occupancy 8 by registers; the LDS path is bound by its dynamic LDS: 10 one-wavefront
// workgroups per CU at R = 0, 6 at R = 16, 3 at R = 64.  No per-lane arrays indexed at run time; every store is a vector store
// from plain C++.
#include <limits.h>

#include "map_descend.hpp"
#include "map_region.hpp"

namespace svoslam {

namespace {

constexpr int kNone = 1 << 30;       // no set bit / no target cell within R so far; kNone + R^2 fits an int32
constexpr int kSeg = 64;             // outputs of one column segment
constexpr int kLdsMaxRadius = 64;    // staged rows <= kSeg + 2 * 64 = 192: 48 KB of LDS per workgroup

__global__ __launch_bounds__(256) void region_raster_kernel(const uint32_t *__restrict__ pool, int d, int x0, int y0, int z0, int x1,
                                                            int wpr, int iny, long long words, bool complement,
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
    target = hit != complement;
  }
  const unsigned long long row_word = __ballot(target);
  if (lane == 0) bits[word] = row_word;
}

template <bool kArg>
__global__ __launch_bounds__(256) void edt_x_kernel(const unsigned long long *__restrict__ bits, int wpr, int nx, int offx, int R,
                                                    long long total, int32_t *__restrict__ g, uint16_t *__restrict__ wit) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= total) return;
  const unsigned long long *__restrict__ w = bits + (idx / nx) * wpr;
  const int p = (int)(idx % nx) + offx, wi = p >> 6, b = p & 63;
  const unsigned long long own = w[wi];
  int best = R + 1, at = p;  // kArg keeps where a strictly nearer bit lies; without it the update is a plain minimum
  unsigned long long m = own & (~0ull >> (63 - b));  // the cell itself and below
  if (m) {
    const int dist = b - (63 - __builtin_clzll(m));
    if constexpr (kArg) { if (dist < best) { best = dist; at = p - dist; } } else best = min(best, dist);
  } else {
    for (int k = 1; k <= wi && b + 1 + 64 * (k - 1) < best; k++) {  // the nearest a bit of word wi - k can be
      const unsigned long long v = w[wi - k];
      if (v) {
        const int dist = b + 1 + 64 * (k - 1) + __builtin_clzll(v);
        if constexpr (kArg) { if (dist < best) { best = dist; at = p - dist; } } else best = min(best, dist);
        break;
      }
    }
  }
  m = own & (~0ull << b);  // the cell itself and above: only what is strictly nearer than the side below
  if (m) {
    const int dist = __builtin_ctzll(m) - b;
    if constexpr (kArg) { if (dist < best) { best = dist; at = p + dist; } } else best = min(best, dist);
  } else {
    for (int k = 1; wi + k < wpr && 64 - b + 64 * (k - 1) < best; k++) {
      const unsigned long long v = w[wi + k];
      if (v) {
        const int dist = 64 - b + 64 * (k - 1) + __builtin_ctzll(v);
        if constexpr (kArg) { if (dist < best) { best = dist; at = p + dist; } } else best = min(best, dist);
        break;
      }
    }
  }
  g[idx] = best <= R ? best * best : kNone;
  if constexpr (kArg) wit[idx] = (uint16_t)at;
}

// in: value j of column (a, x) at in[j * stride_j + a * stride_a + x], j in [0, in_len); output i in [0, out_len) is about input
// i + off and goes to out[i * ostride_j + a * ostride_a + x], with kArg the smallest j of its minimum to arg[the same index].
// Workgroup = (x tile, a, segment), flattened.
template <bool kLds, bool kArg>
__global__ __launch_bounds__(64) void edt_pass_kernel(const int32_t *__restrict__ in, int nx, int xtiles, int na, int in_len, int out_len,
                                                      int off, long long stride_j, long long stride_a, long long ostride_j,
                                                      long long ostride_a, int R, int none_out, int32_t *__restrict__ out,
                                                      uint16_t *__restrict__ arg) {
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
    for (int k = 1; kArg ? k * k <= best : k * k < best; k++) {
      int lo = kNone, hi = kNone;
      if (r - k >= 0) lo = kLds ? seg[(r - k) * 64 + lane] : col[(r - k) * stride_j];
      if (r + k < rows) hi = kLds ? seg[(r + k) * 64 + lane] : col[(r + k) * stride_j];
      if constexpr (kArg) {
        lo += k * k;
        hi += k * k;
        if (lo <= best) { best = lo; at = r - k; }
        if (hi < best) { best = hi; at = r + k; }
      } else {
        best = min(best, min(lo, hi) + k * k);
      }
    }
    o[i * ostride_j] = best < cap ? best : none_out;
    if constexpr (kArg) oa[i * ostride_j] = (uint16_t)(jlo + at);
  }
}

template <bool kOverwrite>
__global__ __launch_bounds__(256) void region_pack_kernel(int32_t *__restrict__ values, int nx, int wpr, long long words, bool invert,
                                                          int none, unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  const long long at = (word / wpr) * nx + x;
  const bool in = x < nx;
  const unsigned long long row_word = __ballot(in && (values[at] == -1) != invert);
  if (kOverwrite && in) values[at] = none;
  if (lane == 0) bits[word] = row_word;
}

// one column pass: the LDS form up to kLdsMaxRadius, staging in_len or kSeg + 2 R rows, whichever is less
template <bool kArg>
int launch_pass(const int32_t *in, long long nx, long long na, long long in_len, long long out_len, int off, long long stride_j,
                long long stride_a, long long ostride_j, long long ostride_a, int R, int none_out, int32_t *out, uint16_t *arg,
                hipStream_t stream) {
  const long long xtiles = (nx + 63) / 64;
  const unsigned blocks = (unsigned)(xtiles * na * ((out_len + kSeg - 1) / kSeg));
  const size_t lds = (size_t)(in_len < kSeg + 2 * R ? in_len : kSeg + 2 * R) * 256;
  if (R <= kLdsMaxRadius)
    edt_pass_kernel<true, kArg><<<blocks, 64, lds, stream>>>(in, (int)nx, (int)xtiles, (int)na, (int)in_len, (int)out_len, off, stride_j,
                                                            stride_a, ostride_j, ostride_a, R, none_out, out, arg);
  else
    edt_pass_kernel<false, kArg><<<blocks, 64, 0, stream>>>(in, (int)nx, (int)xtiles, (int)na, (int)in_len, (int)out_len, off, stride_j,
                                                           stride_a, ostride_j, ostride_a, R, none_out, out, arg);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

template <bool kArg>
int transform(const RegionPlan &p, int R, const unsigned long long *bits, int32_t *g1, int32_t *g2, int32_t *out, uint16_t *wx,
              uint16_t *ay, uint16_t *az, hipStream_t stream, LaunchEvents *timed) {
  const long long nx = p.nx, ny = p.ny;
  if (timed) SVO_TRY(timed->mark(stream));
  edt_x_kernel<kArg><<<cdiv(p.n_g1, 256), 256, 0, stream>>>(bits, (int)p.wpr, (int)nx, p.off[0], R, p.n_g1, g1, wx);
  SVO_LAUNCH_CHECK();
  if (timed) SVO_TRY(timed->mark(stream));
  // y: columns (z of the inflated range, x), g1[z'][y'][x] -> g2[z'][y][x]
  SVO_TRY(launch_pass<kArg>(g1, nx, p.len[2], p.len[1], ny, p.off[1], nx, p.len[1] * nx, nx, ny * nx, R, kNone, g2, ay, stream));
  if (timed) SVO_TRY(timed->mark(stream));
  // z: columns (y, x), g2[z'][y][x] -> out[z][y][x]
  return launch_pass<kArg>(g2, nx, ny, p.len[2], p.nz, p.off[2], ny * nx, nx, ny * nx, nx, R, -1, out, az, stream);
}

}  // namespace

int plan_region(int depth, const int32_t origin[3], const int32_t dims[3], int R, RegionPlan *plan) {
  if (!origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_INVALID_ARG;
  if (R < 0 || R > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // R^2 + 2^30 and 3 R^2 fit an int32
  RegionPlan &p = *plan;
  const long long N = 1ll << depth;
  p.nothing = false;
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > N) return SVOSLAM_ERR_INVALID_ARG;
    p.nothing = p.nothing || dims[a] == 0;
    p.lo[a] = origin[a] - R > 0 ? origin[a] - R : 0;
    const long long end = (long long)origin[a] + dims[a] + R < N ? (long long)origin[a] + dims[a] + R : N;
    p.len[a] = end - p.lo[a];
    p.off[a] = (int)(origin[a] - p.lo[a]);
  }
  p.nx = dims[0], p.ny = dims[1], p.nz = dims[2];  // every side is <= 2^16, so none of these products overflows an int64
  p.n_out = p.nx * p.ny * p.nz;
  p.wpr = (p.len[0] + 63) / 64;
  p.words = p.wpr * p.len[1] * p.len[2];
  p.n_g1 = p.nx * p.len[1] * p.len[2];
  p.n_g2 = p.nx * p.ny * p.len[2];
  return SVOSLAM_OK;
}

int plan_region_axes(int depth, const int32_t origin[3], const int32_t dims[3], const int below[3], const int above[3], int pass_axis,
                     RegionPlan *plan) {
  if (!origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH || (pass_axis != 1 && pass_axis != 2)) return SVOSLAM_ERR_INVALID_ARG;
  RegionPlan &p = *plan;
  const long long N = 1ll << depth;
  p.nothing = false;
  for (int a = 0; a < 3; a++) {
    if (below[a] < 0 || below[a] > SVOSLAM_MAX_RADIUS_CELLS || above[a] < 0 || above[a] > SVOSLAM_MAX_RADIUS_CELLS)
      return SVOSLAM_ERR_INVALID_ARG;
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > N) return SVOSLAM_ERR_INVALID_ARG;
    p.nothing = p.nothing || dims[a] == 0;
    p.lo[a] = origin[a] - below[a] > 0 ? origin[a] - below[a] : 0;
    const long long end = (long long)origin[a] + dims[a] + above[a] < N ? (long long)origin[a] + dims[a] + above[a] : N;
    p.len[a] = end - p.lo[a];
    p.off[a] = (int)(origin[a] - p.lo[a]);
  }
  p.nx = dims[0], p.ny = dims[1], p.nz = dims[2];
  p.n_out = p.nx * p.ny * p.nz;
  p.wpr = (p.len[0] + 63) / 64;
  p.words = p.wpr * p.len[1] * p.len[2];
  p.n_g1 = p.nx * p.len[1] * p.len[2];
  p.n_g2 = pass_axis == 1 ? p.nx * p.ny * p.len[2] : p.nx * p.len[1] * p.nz;
  return SVOSLAM_OK;
}

bool planar_within_limits(const RegionPlan &p, int pass_axis) {
  const long long limit = INT_MAX, xtiles = (p.nx + 63) / 64;
  const long long blocks = pass_axis == 1 ? xtiles * p.len[2] * ((p.ny + kSeg - 1) / kSeg) : xtiles * p.len[1] * ((p.nz + kSeg - 1) / kSeg);
  return p.words <= limit && p.n_g1 <= limit && p.n_g2 <= limit && blocks <= limit;
}

int admit_region(const char *fn, const svoslam_pool *pool, const RegionPlan &p, int R, bool transform, hipStream_t stream) {
  if (!pool || !pool->d_data) return SVOSLAM_ERR_INVALID_ARG;
  const long long limit = INT_MAX, xtiles = (p.nx + 63) / 64;
  if (p.n_out > limit) {
    set_last_error_text("%s: %lld x %lld x %lld cells are more than 2^31 - 1", fn, p.nx, p.ny, p.nz);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (transform && (p.words > limit || p.n_g1 > limit || p.n_g2 > limit || xtiles * p.len[2] * ((p.ny + kSeg - 1) / kSeg) > limit ||
                    xtiles * p.ny * ((p.nz + kSeg - 1) / kSeg) > limit)) {
    set_last_error_text("%s: the region inflated by %d cells (%lld x %lld x %lld) needs an intermediate of more than 2^31 - 1 elements",
                        fn, R, p.len[0], p.len[1], p.len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (p.words > limit) {
    set_last_error_text("%s: the region inflated by %d cells (%lld x %lld x %lld) needs more than 2^31 - 1 row words", fn, R, p.len[0],
                        p.len[1], p.len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // as extract_voxel_grid drains pending asynchronous fusions
  return SVOSLAM_OK;
}

int region_raster(const svoslam_pool *pool, int depth, const RegionPlan &p, bool complement, unsigned long long *bits,
                  hipStream_t stream) {
  region_raster_kernel<<<cdiv(p.words, 4), 256, 0, stream>>>(pool->d_data, depth, (int)p.lo[0], (int)p.lo[1], (int)p.lo[2],
                                                             (int)(p.lo[0] + p.len[0]), (int)p.wpr, (int)p.len[1], p.words, complement,
                                                             bits);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int LaunchEvents::mark(hipStream_t stream) {
  SVO_HIP(hipEventCreate(&ev[n]));
  n++;
  SVO_HIP(hipEventRecord(ev[n - 1], stream));
  return SVOSLAM_OK;
}

LaunchEvents::~LaunchEvents() { for (int k = 0; k < n; k++) (void)hipEventDestroy(ev[k]); }

int region_transform(const RegionPlan &p, int R, const unsigned long long *bits, int32_t *g1, int32_t *g2, int32_t *out, uint16_t *wx,
                     uint16_t *ay, uint16_t *az, hipStream_t stream, LaunchEvents *timed) {
  return wx ? transform<true>(p, R, bits, g1, g2, out, wx, ay, az, stream, timed)
            : transform<false>(p, R, bits, g1, g2, out, nullptr, nullptr, nullptr, stream, timed);
}

int region_transform_planar(const RegionPlan &p, int R, int pass_axis, const unsigned long long *bits, int32_t *g1, int32_t *out,
                            hipStream_t stream) {
  const long long nx = p.nx, ly = p.len[1];
  edt_x_kernel<false><<<cdiv(p.n_g1, 256), 256, 0, stream>>>(bits, (int)p.wpr, (int)nx, p.off[0], R, p.n_g1, g1, nullptr);
  SVO_LAUNCH_CHECK();
  if (pass_axis == 1)  // y: columns (z of the inflated range, x), g1[z'][y'][x] -> out[z'][y][x]
    return launch_pass<false>(g1, nx, p.len[2], ly, p.ny, p.off[1], nx, ly * nx, nx, p.ny * nx, R, -1, out, nullptr, stream);
  // z: columns (y of the inflated range, x), g1[z'][y'][x] -> out[z][y'][x]
  return launch_pass<false>(g1, nx, ly, p.len[2], p.nz, p.off[2], ly * nx, nx, ly * nx, nx, R, -1, out, nullptr, stream);
}

int region_pack(const RegionPlan &own, int32_t *values, bool invert, const int *none, unsigned long long *bits, hipStream_t stream) {
  if (none)
    region_pack_kernel<true><<<cdiv(own.words, 4), 256, 0, stream>>>(values, (int)own.nx, (int)own.wpr, own.words, invert, *none, bits);
  else
    region_pack_kernel<false><<<cdiv(own.words, 4), 256, 0, stream>>>(values, (int)own.nx, (int)own.wpr, own.words, invert, 0, bits);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
