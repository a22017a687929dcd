// map_nearest.hip -- the nearest-cell field of a map region: for every cell of a box of cells the squared distance, in cells, to the
// nearest cell of a target set A within `radius_cells` AND that cell, the witness: the one with the smallest z, then y, then x among
// the equally near (own specification; the restatement the device must equal bit for bit is
// tests/test_nearest_cpu.py).  A is the occupied cells of the root (then the witness's node and colour word can be had too) or the
// cells of the root that are not occupied.  The route is the distance field's exact truncated distance transform with every pass also
// keeping WHERE its minimum lies: map_region.hip's raster (complemented for the free cells), edt_x_kernel<true> and
// edt_pass_kernel<kLds, true>, described there with the tie rule.  This file adds the last step:
//   nearest_resolve_kernel  one lane per output cell follows the three indices: z' from the z pass, y' = the y pass's argmin at
//                           (x, y, z'), x' = the x pass's witness at (x, y', z'); only one 16-bit index per pass is ever stored.
//                           With node / colour asked for, one descent (map_descend.hpp) to (x', y', z') follows; neighbouring lanes
//                           mostly share the witness.  It writes dist2, cell, node and colour, each only if asked for.
// An index is only followed from a value that is not "none", and such a value is a sum whose terms are not "none" either, so
// every index that is read was written (DESIGN.md section 18 has the argument for the tie rule).
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): nearest_resolve_kernel<true> (node / colour) 15 VGPRs,
// <false> 11; 0 bytes of scratch, no LDS, occupancy 8.  Every store is a vector store from plain C++.
#include "map_descend.hpp"
#include "map_nearest.hpp"
#include "map_region.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

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
  if (!ws || (which != SVOSLAM_NEAREST_OCCUPIED && which != SVOSLAM_NEAREST_FREE)) return SVOSLAM_ERR_INVALID_ARG;
  if (which == SVOSLAM_NEAREST_FREE && (d_node || d_color)) return SVOSLAM_ERR_INVALID_ARG;  // a free cell has no level-d node
  RegionPlan p;
  SVO_TRY(plan_region(depth, origin, dims, R, &p));
  if (p.nothing) return SVOSLAM_OK;
  if (!d_dist2 && !d_cell && !d_node && !d_color) return SVOSLAM_ERR_INVALID_ARG;
  SVO_TRY(admit_region("svoslam_pool_nearest_field", pool, p, R, true, stream));
  // one slot for the bit rows, one for the three value arrays (after the x, the y and the z pass), one for their three indices
  int rc = ws->near_bits.reserve((size_t)p.words * 8);
  if (rc == SVOSLAM_OK) rc = ws->near_dist.reserve((size_t)(p.n_g1 + p.n_g2 + p.n_out) * 4);
  if (rc == SVOSLAM_OK) rc = ws->near_arg.reserve((size_t)(p.n_g1 + p.n_g2 + p.n_out) * 2);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->near_bits.release(); ws->near_dist.release(); ws->near_arg.release();
    return rc;
  }
  unsigned long long *bits = ws->near_bits.as<unsigned long long>();
  int32_t *g1 = ws->near_dist.as<int32_t>(), *g2 = g1 + p.n_g1, *g3 = g2 + p.n_g2;
  uint16_t *wx = ws->near_arg.as<uint16_t>(), *ay = wx + p.n_g1, *az = ay + p.n_g2;
  StageScope query(kStageQuery, stream);
  SVO_TRY(region_raster(pool, depth, p, which == SVOSLAM_NEAREST_FREE, bits, stream));
  SVO_TRY(region_transform(p, R, bits, g1, g2, g3, wx, ay, az, stream));
  unsigned long long *cell = reinterpret_cast<unsigned long long *>(d_cell);
  if (d_node || d_color)
    nearest_resolve_kernel<true><<<cdiv(p.n_out, 256), 256, 0, stream>>>(pool->d_data, depth, g3, az, ay, wx, (int)p.nx, (int)p.ny,
                                                                         (int)p.len[1], (int)p.lo[0], (int)p.lo[1], (int)p.lo[2],
                                                                         (int)p.n_out, d_dist2, cell, d_node, d_color);
  else
    nearest_resolve_kernel<false><<<cdiv(p.n_out, 256), 256, 0, stream>>>(pool->d_data, depth, g3, az, ay, wx, (int)p.nx, (int)p.ny,
                                                                          (int)p.len[1], (int)p.lo[0], (int)p.lo[1], (int)p.lo[2],
                                                                          (int)p.n_out, d_dist2, cell, d_node, d_color);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam

