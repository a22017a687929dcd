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
//   reach_seed_kernel   one lane per seed entry: a seed in the region whose bit is set writes 0, is counted, and marks its tile.
//   reach_relax_kernel  one workgroup of 256 per tile of 64 x 8 x 8 cells, launched over all tiles; a tile whose flag of this
//                       round is clear leaves at once.  The tile's steps with a one-cell halo (10 x 10 rows of 66 dwords, 26400
//                       bytes) and its 64 row words are staged in LDS.  One pass = three sweeps, each exact along its axis
//                       (map_sweeps.hpp, with a step of 1 per move):
//                         x  a wavefront per row, a lane per cell: sweep_row, after the two halo cells of the row;
//                         y  a lane per (x, z) column: sweep_column up and down the 8 cells from the halo, x across the lanes;
//                         z  the same per (x, y) column.
//                       In every sweep a lane reads and writes only cells it owns in that sweep (and reads the halo, which nobody
//                       writes), with a barrier between sweeps; rows are at dword row * 66 + 1 + lane: 64 consecutive dwords per
//                       access.  Passes repeat until one changes nothing (a workgroup-wide OR): every pass lowers a value or is the
//                       last.  Then each lane compares its cells with global memory, stores the lowered ones, and the workgroup
//                       raises next round's flag of every face neighbour whose adjoining face it lowered, and the counter of
//                       changed tiles.  Other workgroups read those faces as their halo during the same launch: all global
//                       accesses to the steps are relaxed 32-bit atomics.  Whichever value a neighbour saw, it runs again next
//                       round if the face changed, and values only fall towards the unique fixed point (section 16).
//   reach_finish_kernel "none" becomes -1, a cell without its bit -2.
// The host launches rounds until the counter of changed tiles stands still, reading 32 bytes per round: the call blocks.  No
// cooperative launch, no workgroup waits on another, every device loop ends by its own data, and the rounds are capped.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): reach_relax_kernel 58 VGPRs, 88 SGPRs, 27176 bytes of
// static LDS (6 workgroups per CU of 160 KB), occupancy 6 by registers; reach_finish_kernel 14 VGPRs,
// reach_seed_kernel 12, no LDS, occupancy 8; every kernel 0 bytes of scratch.  No per-lane arrays indexed at run time, no inline
// assembly.
#include <limits.h>

#include "map_field.hpp"
#include "map_reach.hpp"
#include "map_region.hpp"
#include "map_sweeps.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr int kNone = 1 << 30;                 // not reached so far; kNone + 64 fits an int32
constexpr int kTileX = 64, kTileY = 8, kTileZ = 8;
constexpr int kRowPitch = kTileX + 2;          // a staged row: halo, 64 cells, halo
constexpr int kRowsY = kTileY + 2;             // staged rows per z, and kTileZ + 2 of those
constexpr int kStaged = (kTileZ + 2) * kRowsY * kRowPitch;

struct ReachControl {  // the record the host reads once per round
  unsigned long long changed_tiles, tile_runs;  // sums over all rounds so far
  int32_t seeds_used, pad;
};
constexpr size_t kControlBytes = 32;  // the tile flags of the two rounds follow
static_assert(sizeof(ReachControl) <= kControlBytes, "the control record and the flags share a slot");

__device__ inline int load_steps(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_steps(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__global__ __launch_bounds__(256) void reach_seed_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, int nx, int ny,
                                                         int nz, int wpr, int tiles_x, int tiles_y,
                                                         const unsigned long long *__restrict__ bits, int32_t *__restrict__ steps,
                                                         int *__restrict__ flags, ReachControl *__restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, y = (long long)seeds[3 * i + 1] - oy, z = (long long)seeds[3 * i + 2] - oz;
  if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) return;
  const long long row = z * ny + y;
  if (!((bits[row * wpr + (x >> 6)] >> (x & 63)) & 1ull)) return;
  store_steps(steps + row * nx + x, 0);
  atomicAdd(&ctl->seeds_used, 1);
  flags[((z / kTileZ) * tiles_y + y / kTileY) * tiles_x + x / kTileX] = 1;
}

// flags_now: this round's (a tile clears its own), flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void reach_relax_kernel(int32_t *__restrict__ steps, const unsigned long long *__restrict__ bits, int nx,
                                                          int ny, int nz, int wpr, int tiles_x, int tiles_y, int tiles_z,
                                                          int *__restrict__ flags_now, int *__restrict__ flags_next,
                                                          ReachControl *__restrict__ ctl) {
  __shared__ int32_t s[kStaged];
  __shared__ unsigned long long row_bits[kTileZ * kTileY];
  __shared__ int go, faces;
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    go = flags_now[tile];
    flags_now[tile] = 0;
    faces = 0;
  }
  __syncthreads();
  if (!go) return;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / (tiles_x * tiles_y);
  const int x0 = tx * kTileX, y0 = ty * kTileY, z0 = tz * kTileZ;
  const int gx = x0 + lane;

  // stage: staged row r = pz * 10 + py is the row y0 + py - 1, z0 + pz - 1 of the region; outside the region: "none"
  for (int r = w; r < (kTileZ + 2) * kRowsY; r += 4) {
    const int py = r % kRowsY, pz = r / kRowsY;
    const int gy = y0 + py - 1, gz = z0 + pz - 1;
    const bool row_in = gy >= 0 && gy < ny && gz >= 0 && gz < nz;
    const int32_t *__restrict__ row = steps + ((long long)gz * ny + gy) * nx;
    s[r * kRowPitch + 1 + lane] = row_in && gx < nx ? load_steps(row + gx) : kNone;
    if (lane == 0) s[r * kRowPitch] = row_in && x0 > 0 ? load_steps(row + x0 - 1) : kNone;
    if (lane == 63) s[r * kRowPitch + kTileX + 1] = row_in && x0 + kTileX < nx ? load_steps(row + x0 + kTileX) : kNone;
  }
  if (tid < kTileZ * kTileY) {
    const int gy = y0 + (tid & 7), gz = z0 + (tid >> 3);
    row_bits[tid] = gy < ny && gz < nz ? bits[((long long)gz * ny + gy) * wpr + tx] : 0ull;
  }
  __syncthreads();

  int again;
  do {
    int changed = 0;
    // x: a wavefront per row
    for (int r = w; r < kTileZ * kTileY; r += 4) {
      const unsigned long long tw = row_bits[r];
      if (tw == 0ull) continue;  // the same for the whole wavefront
      const int at = (((r >> 3) + 1) * kRowsY + (r & 7) + 1) * kRowPitch + 1 + lane;
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
    for (int z = w; z < kTileZ; z += 4) {
      int32_t *col = s + (z + 1) * kRowsY * kRowPitch + 1 + lane;  // the halo cell below the column; the one above is 9 rows on
      changed |= sweep_column<1, kNone, kRowPitch, 1, true>(col + kRowPitch, row_bits + z * 8, lane, col[0]);
      changed |= sweep_column<1, kNone, kRowPitch, 1, false>(col + kRowPitch, row_bits + z * 8, lane, col[(kTileY + 1) * kRowPitch]);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileY; y += 4) {
      constexpr int kPlane = kRowsY * kRowPitch;
      int32_t *col = s + (y + 1) * kRowPitch + 1 + lane;
      changed |= sweep_column<1, kNone, kPlane, 8, true>(col + kPlane, row_bits + y, lane, col[0]);
      changed |= sweep_column<1, kNone, kPlane, 8, false>(col + kPlane, row_bits + y, lane, col[(kTileZ + 1) * kPlane]);
    }
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  // write back what fell; which faces towards an existing neighbour tile fell
  int mine = 0;
  for (int r = w; r < kTileZ * kTileY; r += 4) {
    const int y = r & 7, z = r >> 3;
    if (!((row_bits[r] >> lane) & 1ull)) continue;  // a set bit: the cell is inside the region
    const int v = s[((z + 1) * kRowsY + y + 1) * kRowPitch + 1 + lane];
    int32_t *p = steps + ((long long)(z0 + z) * ny + (y0 + y)) * nx + gx;
    if (v < load_steps(p)) {
      store_steps(p, v);
      mine |= 64;
      if (lane == 0 && tx > 0) mine |= 1;
      if (lane == 63 && tx + 1 < tiles_x) mine |= 2;
      if (y == 0 && ty > 0) mine |= 4;
      if (y == kTileY - 1 && ty + 1 < tiles_y) mine |= 8;
      if (z == 0 && tz > 0) mine |= 16;
      if (z == kTileZ - 1 && tz + 1 < tiles_z) mine |= 32;
    }
  }
  if (mine) atomicOr(&faces, mine);
  __syncthreads();
  if (tid == 0) {
    const int f = faces;
    if (f & 1) flags_next[tile - 1] = 1;
    if (f & 2) flags_next[tile + 1] = 1;
    if (f & 4) flags_next[tile - tiles_x] = 1;
    if (f & 8) flags_next[tile + tiles_x] = 1;
    if (f & 16) flags_next[tile - tiles_x * tiles_y] = 1;
    if (f & 32) flags_next[tile + tiles_x * tiles_y] = 1;
    if (f) atomicAdd(&ctl->changed_tiles, 1ull);
    atomicAdd(&ctl->tile_runs, 1ull);
  }
}

__global__ __launch_bounds__(256) void reach_finish_kernel(int32_t *__restrict__ steps, int nx, int wpr, long long words,
                                                           const unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  if (x >= nx) return;
  const long long at = (word / wpr) * nx + x;
  const int v = steps[at];
  steps[at] = !((bits[word] >> lane) & 1ull) ? -2 : v == kNone ? -1 : v;
}

}  // namespace

int pool_reach_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t r, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_steps, svoslam_reach_stats *stats,
                     hipStream_t stream) {
  if (stats) stats->rounds = stats->tile_runs = stats->seeds_used = 0;
  if (!ws || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || n_seeds < 0 || (n_seeds > 0 && !d_seeds)) return SVOSLAM_ERR_INVALID_ARG;
  RegionPlan own;  // the region itself: its row words are <= the field's own, within its limits
  SVO_TRY(plan_region(depth, origin, dims, 0, &own));
  if (own.nothing) return SVOSLAM_OK;
  const long long nx = own.nx, ny = own.ny, nz = own.nz, wpr = own.wpr, words = own.words;
  const long long tiles_x = wpr, tiles_y = (ny + kTileY - 1) / kTileY, tiles_z = (nz + kTileZ - 1) / kTileZ;
  const long long tiles = tiles_x * tiles_y * tiles_z;
  // a launch takes at most 2^32 - 1 work-items: decided here, before anything is allocated or written
  if (own.n_out <= INT_MAX && tiles * 256 > 0xFFFFFFFFll) {
    set_last_error_text("svoslam_pool_reach_field: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)", nx,
                        ny, nz, tiles);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  // the traversable set, as the field's -1, in d_steps: the rest of the argument checks, the field's limits (decided before
  // anything is allocated), the drain of pending fusions and the field's own slots are pool_distance_field's
  SlotRollback grown(ws, &ws->reach_bits, &ws->reach_flags);
  AdoptedBracket bracket(stream);
  SVO_TRY(pool_distance_field(ws, pool, depth, origin, dims, r, d_steps, nullptr, stream, &bracket.token));
  int rc = ws->reach_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->reach_flags.reserve(kControlBytes + (size_t)tiles * 8);
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  unsigned long long *bits = ws->reach_bits.as<unsigned long long>();
  ReachControl *ctl = ws->reach_flags.as<ReachControl>();
  int *flags = reinterpret_cast<int *>(ws->reach_flags.as<char>() + kControlBytes);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + (size_t)tiles * 8, stream));
  SVO_TRY(region_pack(own, d_steps, false, &kNone, bits, stream));  // d_steps becomes the working array in place
  if (n_seeds > 0) {
    reach_seed_kernel<<<cdiv(n_seeds, 256), 256, 0, stream>>>(d_seeds, n_seeds, origin[0], origin[1], origin[2], (int)nx, (int)ny, (int)nz,
                                                              (int)wpr, (int)tiles_x, (int)tiles_y, bits, d_steps, flags, ctl);
    SVO_LAUNCH_CHECK();
  }
  // rounds: a round in which no tile lowered anything is the last.  After round k every cell whose shortest path crosses at most
  // k tile faces is final, and a path has fewer cells than the region, so the cap below is never reached; it keeps the loop from
  // spinning whatever happens.
  const long long cap = tiles * (long long)(kTileX * kTileY * kTileZ) + 1;
  ReachControl seen = {};
  unsigned long long changed_before = 0;
  long long rounds = 0;
  for (;;) {
    if (rounds >= cap) {
      set_last_error_text("svoslam_pool_reach_field: no convergence after %lld rounds over %lld tiles", rounds, tiles);
      return SVOSLAM_ERR_HIP;
    }
    int *now = flags + (rounds & 1) * tiles, *next = flags + ((rounds + 1) & 1) * tiles;
    reach_relax_kernel<<<(unsigned)tiles, 256, 0, stream>>>(d_steps, bits, (int)nx, (int)ny, (int)nz, (int)wpr, (int)tiles_x, (int)tiles_y,
                                                            (int)tiles_z, now, next, ctl);
    SVO_LAUNCH_CHECK();
    rounds++;
    SVO_HIP(hipMemcpyAsync(&seen, ctl, sizeof(seen), hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    if (seen.changed_tiles == changed_before) break;
    changed_before = seen.changed_tiles;
  }
  reach_finish_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_steps, (int)nx, (int)wpr, words, bits);
  SVO_LAUNCH_CHECK();
  if (stats) {
    stats->rounds = (int32_t)(rounds < INT_MAX ? rounds : INT_MAX);
    stats->tile_runs = (int32_t)(seen.tile_runs < (unsigned long long)INT_MAX ? seen.tile_runs : (unsigned long long)INT_MAX);
    stats->seeds_used = seen.seeds_used;
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
