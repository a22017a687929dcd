// map_plan.hip -- path planning in a map region (own specification, DESIGN.md section 21: the reference has nothing like it; the
// restatements the device must equal value for value are in tests/test_plan_cpu.py).
//
// pool_cost_field: the reach field (map_reach.hip, section 16) with a weight per cell.  A cell is traversable iff no occupied cell
// lies within clearance_cells = r of it; entering a traversable cell q costs w(q) = 1 + ring_cost[j - r - 1], where j is the ring
// (j - 1)^2 < D <= j^2 of its squared distance D to the nearest occupied cell, or 1 beyond comfort_cells = R.  The value of a cell
// is the cheapest sum of w over the cells of a path from a seed, the seed itself left out; -1 without a path, -2 where the cell is
// not traversable.  The distance field with radius R is computed first, by the existing host function, into d_cost itself.
//
//   plan_weigh_kernel   one wavefront per 64 x of a row: every lane turns its dist2 into "traversable" and w (an integer
//                       ceil-sqrt: the correctly rounded binary32 root of D <= 2^24, corrected in integers); the ballot is the
//                       row word, the weight goes to its 16-bit slot, and the lane overwrites its dist2 with "none" (2^30):
//                       d_cost becomes the working array in place.
//   the seeds, the rounds, the finish: map_relax.hpp's scheme, as the reach field uses it (x, y, z; a one-cell halo).
//   plan_relax_kernel   what is the cost field's own in a round.  Staged in LDS beside the tile's costs (26400 bytes) and its 64
//                       row words: the 16-bit weights of its OWN cells (8192 bytes) -- a move is charged the weight of the cell
//                       it enters, so the halo needs none.  One pass = three sweeps (map_sweeps.hpp): x a segmented min-plus scan
//                       on prefix sums of the row's weights (sweep_row_weighted), the halo entering lanes 0 and 63 as halo +
//                       w(own cell); y and z serial over 8 cells with the cell's weight (sweep_column_weighted).  Passes repeat
//                       until one changes nothing.
//
// field_trace_paths: trace_paths_kernel, one lane per start: from a cell of value v > 0 to the face neighbour inside the region
// with the smallest value 0 <= v' < v (the first of -x +x -y +y -z +z on a tie), until a cell of value 0.  The values fall
// strictly, so the walk is bounded by its data; it is a chain of dependent loads, and a lane per start keeps many chains in flight.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): plan_relax_kernel 67 VGPRs, 86 SGPRs, 35368 bytes of
// static LDS (4 workgroups per CU of 160 KB), occupancy 4 by LDS; plan_weigh_kernel 14 VGPRs,
// trace_paths_kernel 26 VGPRs and 58 SGPRs, no LDS, occupancy 8; every kernel 0 bytes of scratch.  No per-lane arrays indexed at run
// time, no inline assembly.
#include "map_field.hpp"
#include "map_plan.hpp"
#include "map_region.hpp"
#include "map_relax.hpp"
#include "map_sweeps.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

// values: dist2 with radius R (-1: beyond R) on the way in, "none" on the way out.  ring[j - r - 1]: the cost of ring j, r < j <= R
__global__ __launch_bounds__(256) void plan_weigh_kernel(int32_t *__restrict__ values, int nx, int wpr, long long words, int r, int R,
                                                         const int32_t *__restrict__ ring, unsigned long long *__restrict__ bits,
                                                         uint16_t *__restrict__ weights) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  const long long at = (word / wpr) * nx + x;
  const bool in = x < nx;
  bool free_cell = false;
  int wt = 1;
  if (in) {
    const int D = values[at];
    free_cell = D < 0 || D > r * r;
    if (free_cell && D >= 0 && R > r) {  // r^2 < D <= R^2: the ring j with (j - 1)^2 < D <= j^2
      int j = (int)ceilf(sqrtf((float)D));
      if ((j - 1) * (j - 1) >= D) j--;
      if (j * j < D) j++;
      j = min(max(j, r + 1), R);
      wt = 1 + ring[j - r - 1];
    }
    values[at] = kNone;
    weights[at] = (uint16_t)wt;
  }
  const unsigned long long row_word = __ballot(free_cell);
  if (lane == 0) bits[word] = row_word;
}

// flags_now: this round's, flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void plan_relax_kernel(int32_t *__restrict__ cost, const unsigned long long *__restrict__ bits,
                                                         const uint16_t *__restrict__ weights, TileGrid g, int *__restrict__ flags_now,
                                                         int *__restrict__ flags_next, RelaxControl *__restrict__ ctl) {
  __shared__ int32_t s[(kTileB + 2) * kLayer];
  __shared__ uint16_t wts[kTileRows * kTileX];  // the tile's own cells: row r = z * 8 + y at r * 64
  __shared__ unsigned long long row_bits[kTileRows];
  __shared__ TileShared sh;
  if (!relax_enter(sh, flags_now)) return;
  const TileAt t = tile_at(g);
  relax_stage(s, row_bits, cost, bits, g, t, 1);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int r = w; r < kTileRows; r += 4) {
    const int gx = t.x0 + lane, gy = t.a0 + (r & 7), gz = t.b0 + (r >> 3);
    wts[r * kTileX + lane] = gy < g.na && gz < g.nb && gx < g.nx ? weights[(long long)gy * g.sa + (long long)gz * g.sb + gx] : (uint16_t)0;
  }
  __syncthreads();

  int again;
  do {
    int changed = 0;
    // x: a wavefront per row
    for (int r = w; r < kTileRows; r += 4) {
      const unsigned long long tw = row_bits[r];
      if (tw == 0ull) continue;  // the same for the whole wavefront
      const int at = staged_at(r & 7, r >> 3, 1) + lane;
      const bool set = (tw >> lane) & 1ull;
      const int wt = set ? (int)wts[r * kTileX + lane] : 0;
      const int before = s[at];
      int v = before;
      if (lane == 0) v = min(v, s[at - 1] + wt);
      if (lane == 63) v = min(v, s[at + 1] + wt);
      if (!set) v = kNone;
      v = sweep_row_weighted(v, wt, tw, lane);
      if (v < before) { s[at] = v; changed = 1; }
    }
    __syncthreads();
    // y: a lane per (x, z) column
    for (int z = w; z < kTileB; z += 4) {
      int32_t *col = s + (z + 1) * kLayer + 1 + lane;  // the halo cell below the column; the one above is 9 rows on
      const uint16_t *cw = wts + z * kTileA * kTileX + lane;
      changed |= sweep_column_weighted<kNone, kRowPitch, 1, kTileX, true>(col + kRowPitch, row_bits + z * 8, cw, lane, col[0]);
      changed |= sweep_column_weighted<kNone, kRowPitch, 1, kTileX, false>(col + kRowPitch, row_bits + z * 8, cw, lane,
                                                                           col[(kTileA + 1) * kRowPitch]);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileA; y += 4) {
      int32_t *col = s + (y + 1) * kRowPitch + 1 + lane;
      const uint16_t *cw = wts + y * kTileX + lane;
      changed |= sweep_column_weighted<kNone, kLayer, 8, kTileA * kTileX, true>(col + kLayer, row_bits + y, cw, lane, col[0]);
      changed |= sweep_column_weighted<kNone, kLayer, 8, kTileA * kTileX, false>(col + kLayer, row_bits + y, cw, lane,
                                                                                 col[(kTileB + 1) * kLayer]);
    }
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  relax_store_faces(cost, s, row_bits, sh, g, t, flags_next, ctl);
}

// one lane per start.  Every index read lies inside the region: a neighbour is looked at only after its coordinate was tested.
__global__ __launch_bounds__(256) void trace_paths_kernel(const int32_t *__restrict__ field, long long ox, long long oy, long long oz,
                                                          long long nx, long long ny, long long nz, const int32_t *__restrict__ starts, int n,
                                                          int max_cells, int32_t *__restrict__ paths, int32_t *__restrict__ lengths) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long x = (long long)starts[3 * i] - ox, y = (long long)starts[3 * i + 1] - oy, z = (long long)starts[3 * i + 2] - oz;
  int len = 0;
  if (x >= 0 && x < nx && y >= 0 && y < ny && z >= 0 && z < nz) {
    const long long sy = nx, sz = nx * ny;
    long long at = z * sz + y * sy + x;
    int v = field[at];
    int32_t *out = paths + (long long)i * max_cells * 3;
    while (v >= 0) {  // v falls strictly with every move and stays >= 0
      if (len < max_cells) {
        out[3 * len] = (int32_t)(x + ox);
        out[3 * len + 1] = (int32_t)(y + oy);
        out[3 * len + 2] = (int32_t)(z + oz);
      }
      len++;
      if (v == 0) break;
      int best = v, dir = -1, u;
      if (x > 0 && (u = field[at - 1]) >= 0 && u < best) { best = u; dir = 0; }
      if (x + 1 < nx && (u = field[at + 1]) >= 0 && u < best) { best = u; dir = 1; }
      if (y > 0 && (u = field[at - sy]) >= 0 && u < best) { best = u; dir = 2; }
      if (y + 1 < ny && (u = field[at + sy]) >= 0 && u < best) { best = u; dir = 3; }
      if (z > 0 && (u = field[at - sz]) >= 0 && u < best) { best = u; dir = 4; }
      if (z + 1 < nz && (u = field[at + sz]) >= 0 && u < best) { best = u; dir = 5; }
      if (dir < 0) { len = -len; break; }  // not a cost-to-go field: a cell above 0 without a lower neighbour
      if (dir == 0) { x--; at--; }
      else if (dir == 1) { x++; at++; }
      else if (dir == 2) { y--; at -= sy; }
      else if (dir == 3) { y++; at += sy; }
      else if (dir == 4) { z--; at -= sz; }
      else { z++; at += sz; }
      v = best;
    }
  }
  lengths[i] = len;
}

}  // namespace

int pool_cost_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3], int32_t r,
                    int32_t R, const int32_t *h_ring_cost, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_cost,
                    svoslam_plan_stats *stats, hipStream_t stream) {
  const char *fn = "svoslam_pool_cost_field";
  if (stats) stats->rounds = stats->tile_runs = stats->seeds_used = stats->max_weight = 0;
  if (!ws || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || R < r || R > SVOSLAM_MAX_RADIUS_CELLS || n_seeds < 0 || (n_seeds > 0 && !d_seeds) ||
      (R > r && !h_ring_cost))
    return SVOSLAM_ERR_INVALID_ARG;
  const int rings = R - r;
  long long max_weight = 1;
  for (int k = 0; k < rings; k++) {
    if (h_ring_cost[k] < 0 || h_ring_cost[k] > SVOSLAM_MAX_RING_COST) return SVOSLAM_ERR_INVALID_ARG;
    if (1 + (long long)h_ring_cost[k] > max_weight) max_weight = 1 + (long long)h_ring_cost[k];
  }
  if (stats) stats->max_weight = (int32_t)max_weight;
  RegionPlan own;  // the region itself: its row words are <= the field's own, within its limits
  SVO_TRY(plan_region(depth, origin, dims, 0, &own));
  if (own.nothing) return SVOSLAM_OK;
  const TileGrid g = tile_grid(own.nx, own.ny, own.nz, own.nx, own.nx * own.ny, 1, own.ny, own.wpr);
  const long long tiles = g.tiles(), words = own.words;
  // decided here, before anything is allocated or written: a launch takes at most 2^32 - 1 work-items, and every finite cost has
  // to stay below "none" -- a path has fewer cells than the region, each at most max_weight
  if (own.n_out <= INT_MAX) SVO_TRY(relax_tile_limit(fn, g, own.ny, own.nz));
  if (own.n_out <= INT_MAX && own.n_out * max_weight >= (long long)kNone) {
    set_last_error_text("svoslam_pool_cost_field: %lld cells of weight up to %lld could cost 2^30 or more, the value of \"not reached\"",
                        own.n_out, max_weight);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  // the squared distances within R, in d_cost: the rest of the argument checks, the field's limits (decided before anything is
  // allocated), the drain of pending fusions and the field's own slots are pool_distance_field's
  SlotRollback grown(ws, &ws->plan_bits, &ws->plan_weights, &ws->plan_ctl);
  AdoptedBracket bracket(stream);
  SVO_TRY(pool_distance_field(ws, pool, depth, origin, dims, R, d_cost, nullptr, stream, &bracket.token));
  const size_t flag_bytes = (size_t)tiles * 8;
  int rc = ws->plan_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->plan_weights.reserve((size_t)own.n_out * 2);
  if (rc == SVOSLAM_OK) rc = ws->plan_ctl.reserve(kControlBytes + flag_bytes + (size_t)rings * 4);
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  unsigned long long *bits = ws->plan_bits.as<unsigned long long>();
  uint16_t *weights = ws->plan_weights.as<uint16_t>();
  RelaxControl *ctl = ws->plan_ctl.as<RelaxControl>();
  int *flags = reinterpret_cast<int *>(ws->plan_ctl.as<char>() + kControlBytes);
  int32_t *ring = reinterpret_cast<int32_t *>(ws->plan_ctl.as<char>() + kControlBytes + flag_bytes);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + flag_bytes, stream));
  if (rings > 0) SVO_HIP(hipMemcpyAsync(ring, h_ring_cost, (size_t)rings * 4, hipMemcpyHostToDevice, stream));
  plan_weigh_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_cost, g.nx, g.wpr, words, r, R, ring, bits, weights);
  SVO_LAUNCH_CHECK();  // d_cost has become the working array in place
  SVO_TRY(relax_seed(d_seeds, n_seeds, origin, g, bits, d_cost, flags, ctl, stream));
  long long rounds;
  RelaxControl seen;
  SVO_TRY(relax_rounds(fn, tiles, ctl, flags, stream, [&](int *now, int *next) {
    plan_relax_kernel<<<(unsigned)tiles, 256, 0, stream>>>(d_cost, bits, weights, g, now, next, ctl);
  }, &rounds, &seen));
  SVO_TRY(relax_finish(d_cost, own.nx, own.wpr, words, bits, stream));
  if (stats) relax_stats(stats, rounds, seen);
  return SVOSLAM_OK;
}

int field_trace_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], const int32_t *d_starts, int32_t n_starts,
                      int32_t max_cells, int32_t *d_paths, int32_t *d_lengths, hipStream_t stream) {
  bool launch;
  SVO_TRY(trace_arguments("svoslam_field_trace_paths", d_field, origin, dims, d_starts, n_starts, max_cells, d_paths, d_lengths, &launch));
  if (!launch) return SVOSLAM_OK;
  StageScope timed(kStageQuery, stream);
  trace_paths_kernel<<<cdiv(n_starts, 256), 256, 0, stream>>>(d_field, origin[0], origin[1], origin[2], dims[0], dims[1], dims[2], d_starts,
                                                              n_starts, max_cells, d_paths, d_lengths);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
