// map_field.hip -- the distance field of a map region: for every cell of a box of cells the squared distance, in cells, to the
// nearest occupied cell of the whole root if that is within `radius_cells`, else -1 (own specification, DESIGN.md section 15: the
// reference has nothing like it; the restatement the device must equal bit for bit is tests/test_field_cpu.py).  The value is
// svoslam_pool_nearest_occupied's dist2 for a point inside the cell; it is computed for all cells at once by an exact Euclidean
// distance transform truncated at R, in integers: the occupied set of the region inflated by R is rasterised once and three
// separable passes follow.  The plan of the inflated region, the raster and the transform are map_region.hip's (region_raster_kernel,
// edt_x_kernel<false>, edt_pass_kernel<kLds, false>; their description and resource report are there); this file is the call.
// svoslam_pool_distance_field_profile is the same call with an event around each launch (blocking).
#include "lattice.hpp"
#include "map_field.hpp"
#include "map_region.hpp"
#include "stage_timing.hpp"

namespace svoslam {

int pool_distance_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                        int32_t R, int32_t *d_dist2, float *launch_ms, hipStream_t stream, long long *outer_bracket) {
  if (launch_ms) launch_ms[0] = launch_ms[1] = launch_ms[2] = launch_ms[3] = 0.0f;
  if (!ws) return SVOSLAM_ERR_INVALID_ARG;
  RegionPlan p;
  SVO_TRY(plan_region(depth, origin, dims, R, &p));
  if (p.nothing) return SVOSLAM_OK;
  if (!d_dist2) return SVOSLAM_ERR_INVALID_ARG;
  SVO_TRY(admit_region("svoslam_pool_distance_field", pool, p, R, true, stream));
  int rc = ws->field_bits.reserve((size_t)p.words * 8);
  if (rc == SVOSLAM_OK) rc = ws->field_a.reserve((size_t)p.n_g1 * 4);
  if (rc == SVOSLAM_OK) rc = ws->field_b.reserve((size_t)p.n_g2 * 4);
  if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
    ws->field_bits.release(); ws->field_a.release(); ws->field_b.release();
    return rc;
  }
  unsigned long long *bits = ws->field_bits.as<unsigned long long>();
  LaunchEvents events, *timed = launch_ms ? &events : nullptr;
  // a caller that goes on after the field (map_reach.hip) owns the bracket: it is opened here, where nothing can be refused any
  // more, and closed by the caller
  if (outer_bracket) (void)stage_begin(kStageQuery, stream, outer_bracket);
  StageScope query(outer_bracket ? -1 : (int)kStageQuery, stream);
  if (timed) SVO_TRY(timed->mark(stream));
  SVO_TRY(region_raster(pool, depth, p, false, bits, stream));
  SVO_TRY(region_transform(p, R, bits, ws->field_a.as<int32_t>(), ws->field_b.as<int32_t>(), d_dist2, nullptr, nullptr, nullptr, stream,
                           timed));
  if (timed) {  // the profiling form blocks
    SVO_TRY(timed->mark(stream));
    SVO_HIP(hipEventSynchronize(timed->ev[4]));
    for (int k = 0; k < 4; k++) SVO_HIP(hipEventElapsedTime(&launch_ms[k], timed->ev[k], timed->ev[k + 1]));
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
