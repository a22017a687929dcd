// map_reach.hip -- the reach field of a map region: for every cell of a box of cells the number of face-neighbour moves of the
// shortest path from any seed cell through traversable cells of the region, -1 where there is no such path, -2 where the cell is
// not traversable (own specification, DESIGN.md section 16: the reference has nothing like it; the restatement the device must
// equal value for value is tests/test_reach_cpu.py).  A cell is traversable iff svoslam_pool_distance_field with R =
// clearance_cells writes -1 there, so the field is computed first, by the existing host function and its kernels, into d_steps
// itself; everything after it is integers on the region.
//
//   the pack            map_region.hip's region_pack_kernel<true>: the row words of the traversable bits (dist2 == -1), for the
//                       region itself; every lane then overwrites its own dist2 with "none" (2^30): d_steps becomes the working
//                       array in place, and no slot of the size of the output is needed.
//   the seeds, the rounds, the finish: map_relax.hpp's scheme (tiles of 64 x 8 x 8 cells over x, y, z with a one-cell halo, 10 x 10
//                       rows of 66 dwords, 26400 bytes; flags per tile and round; one 32-byte readback per round).
//   reach_relax_kernel  what is the reach field's own in a round: one pass over the staged tile = three sweeps, each exact along
//                       its axis (map_sweeps.hpp, with a step of 1 per move):
//                         x  a wavefront per row, a lane per cell: sweep_row, after the two halo cells of the row;
//                         y  a lane per (x, z) column: sweep_column up and down the 8 cells from the halo, x across the lanes;
//                         z  the same per (x, y) column.
//                       In every sweep a lane reads and writes only cells it owns in that sweep (and reads the halo, which nobody
//                       writes), with a barrier between sweeps; rows are at dword row * 66 + 1 + lane: 64 consecutive dwords per
//                       access.  Passes repeat until one changes nothing (a workgroup-wide OR): every pass lowers a value or is the
//                       last.
// The host function is reach_relax with relax_seed as its seeding; the owner field (map_owner.hip) runs the same relaxation behind
// a seeding of its own.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): reach_relax_kernel 56 VGPRs, 90 SGPRs, 27176 bytes of
// static LDS (6 workgroups per CU of 160 KB), occupancy 6 by registers; 0 bytes of scratch.  No per-lane arrays indexed at run
// time, no inline assembly.
#include "map_field.hpp"
#include "map_reach.hpp"
#include "map_region.hpp"
#include "map_relax.hpp"
#include "map_sweeps.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

// flags_now: this round's, flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void reach_relax_kernel(int32_t *__restrict__ steps, const unsigned long long *__restrict__ bits, TileGrid g,
                                                          int *__restrict__ flags_now, int *__restrict__ flags_next,
                                                          RelaxControl *__restrict__ ctl) {
  __shared__ int32_t s[(kTileB + 2) * kLayer];
  __shared__ unsigned long long row_bits[kTileRows];
  __shared__ TileShared sh;
  if (!relax_enter(sh, flags_now)) return;
  const TileAt t = tile_at(g);
  relax_stage(s, row_bits, steps, bits, g, t, 1);
  __syncthreads();

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int again;
  do {
    int changed = 0;
    // x: a wavefront per row
    for (int r = w; r < kTileRows; r += 4) {
      const unsigned long long tw = row_bits[r];
      if (tw == 0ull) continue;  // the same for the whole wavefront
      const int at = staged_at(r & 7, r >> 3, 1) + lane;
      const int before = s[at];
      int v = before;
      if (lane == 0) v = min(v, s[at - 1] + 1);
      if (lane == 63) v = min(v, s[at + 1] + 1);
      if (!((tw >> lane) & 1ull)) v = kNone;
      v = sweep_row<1>(v, tw, lane);
      if (v < before) { s[at] = v; changed = 1; }
    }
    __syncthreads();
    // y: a lane per (x, z) column
    for (int z = w; z < kTileB; z += 4) {
      int32_t *col = s + (z + 1) * kLayer + 1 + lane;  // the halo cell below the column; the one above is 9 rows on
      changed |= sweep_column<1, kNone, kRowPitch, 1, true>(col + kRowPitch, row_bits + z * 8, lane, col[0]);
      changed |= sweep_column<1, kNone, kRowPitch, 1, false>(col + kRowPitch, row_bits + z * 8, lane, col[(kTileA + 1) * kRowPitch]);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileA; y += 4) {
      int32_t *col = s + (y + 1) * kRowPitch + 1 + lane;
      changed |= sweep_column<1, kNone, kLayer, 8, true>(col + kLayer, row_bits + y, lane, col[0]);
      changed |= sweep_column<1, kNone, kLayer, 8, false>(col + kLayer, row_bits + y, lane, col[(kTileB + 1) * kLayer]);
    }
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  relax_store_faces(steps, s, row_bits, sh, g, t, flags_next, ctl);
}

}  // namespace

int reach_relax(const char *fn, svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3],
                const int32_t dims[3], int32_t r, int32_t *d_steps, int spare, const std::function<int(const ReachFrame &)> &seed,
                AdoptedBracket &bracket, ReachFrame *frame, long long *rounds, RelaxControl *seen, hipStream_t stream) {
  ReachFrame &f = *frame;
  RegionPlan &own = f.own;  // the region itself: its row words are <= the field's own, within its limits
  SVO_TRY(plan_region(depth, origin, dims, 0, &own));
  if (own.nothing) return SVOSLAM_OK;
  const TileGrid g = f.g = tile_grid(own.nx, own.ny, own.nz, own.nx, own.nx * own.ny, 1, own.ny, own.wpr);
  const long long tiles = f.tiles = g.tiles();
  // decided here, before anything is allocated or written
  if (own.n_out <= INT_MAX) SVO_TRY(relax_tile_limit(fn, g, own.ny, own.nz));
  // the traversable set, as the field's -1, in d_steps: the rest of the argument checks, the field's limits (decided before
  // anything is allocated), the drain of pending fusions and the field's own slots are pool_distance_field's
  SlotRollback grown(ws, &ws->reach_bits, &ws->reach_flags);
  SVO_TRY(pool_distance_field(ws, pool, depth, origin, dims, r, d_steps, nullptr, stream, &bracket.token));
  int rc = ws->reach_bits.reserve((size_t)own.words * 8);
  if (rc == SVOSLAM_OK) rc = ws->reach_flags.reserve(kControlBytes + (size_t)tiles * 4 * (2 + spare));
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  unsigned long long *bits = f.bits = ws->reach_bits.as<unsigned long long>();
  RelaxControl *ctl = f.ctl = ws->reach_flags.as<RelaxControl>();
  int *flags = f.flags = reinterpret_cast<int *>(ws->reach_flags.as<char>() + kControlBytes);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + (size_t)tiles * 8, stream));
  SVO_TRY(region_pack(own, d_steps, false, &kNone, bits, stream));  // d_steps becomes the working array in place
  SVO_TRY(seed(f));
  SVO_TRY(relax_rounds(fn, tiles, ctl, flags, stream, [&](int *now, int *next) {
    reach_relax_kernel<<<(unsigned)tiles, 256, 0, stream>>>(d_steps, bits, g, now, next, ctl);
  }, rounds, seen));
  SVO_TRY(relax_finish(d_steps, own.nx, own.wpr, own.words, bits, stream));
  return SVOSLAM_OK;
}

int pool_reach_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t r, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_steps, svoslam_reach_stats *stats,
                     hipStream_t stream) {
  if (stats) stats->rounds = stats->tile_runs = stats->seeds_used = 0;
  if (!ws || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || n_seeds < 0 || (n_seeds > 0 && !d_seeds)) return SVOSLAM_ERR_INVALID_ARG;
  AdoptedBracket bracket(stream);
  ReachFrame frame;
  long long rounds;
  RelaxControl seen;
  SVO_TRY(reach_relax("svoslam_pool_reach_field", ws, pool, depth, origin, dims, r, d_steps, 0, [&](const ReachFrame &f) {
    return relax_seed(d_seeds, n_seeds, origin, f.g, f.bits, d_steps, f.flags, f.ctl, stream);
  }, bracket, &frame, &rounds, &seen, stream));
  if (stats && !frame.own.nothing) relax_stats(stats, rounds, seen);
  return SVOSLAM_OK;
}

}  // namespace svoslam
