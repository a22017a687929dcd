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
//   plan_seed_kernel    one lane per seed entry: a seed in the region whose bit is set writes 0, is counted, and marks its tile.
//   plan_relax_kernel   the reach field's scheme unchanged: one workgroup of 256 per tile of 64 x 8 x 8 cells, launched over all
//                       tiles, a tile whose flag of this round is clear leaves at once.  Staged in LDS: the tile's costs with a
//                       one-cell halo (26400 bytes), its 64 row words and the 16-bit weights of its OWN cells (8192 bytes) --
//                       a move is charged the weight of the cell it enters, so the halo needs none.  One pass = three sweeps
//                       (map_sweeps.hpp): x a segmented min-plus scan on prefix sums of the row's weights (sweep_row_weighted),
//                       the halo entering lanes 0 and 63 as halo + w(own cell); y and z serial over 8 cells with the cell's
//                       weight (sweep_column_weighted).  Passes repeat until one changes nothing; then the lowered cells are
//                       stored, next round's flag of every face neighbour whose adjoining face fell is raised, and the counter
//                       of changed tiles.  All global accesses to the costs are relaxed 32-bit agent-scope atomics.
//   plan_finish_kernel  "none" becomes -1, a cell without its bit -2.
// The host launches rounds until the counter of changed tiles stands still, reading 32 bytes per round: the call blocks.  No
// cooperative launch, no workgroup waits on another, every device loop ends by its own data, and the rounds are capped.
//
// field_trace_paths: trace_paths_kernel, one lane per start: from a cell of value v > 0 to the face neighbour inside the region
// with the smallest value 0 <= v' < v (the first of -x +x -y +y -z +z on a tie), until a cell of value 0.  The values fall
// strictly, so the walk is bounded by its data; it is a chain of dependent loads, and a lane per start keeps many chains in flight.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): plan_relax_kernel 68 VGPRs, 84 SGPRs, 35368 bytes of
// static LDS (4 workgroups per CU of 160 KB), occupancy 4 by LDS; plan_weigh_kernel and plan_finish_kernel 14 VGPRs, plan_seed_kernel 12,
// trace_paths_kernel 26 VGPRs and 58 SGPRs, no LDS, occupancy 8; every kernel 0 bytes of scratch.  No per-lane arrays indexed at run
// time, no inline assembly.
#include <limits.h>

#include "map_field.hpp"
#include "map_plan.hpp"
#include "map_region.hpp"
#include "map_sweeps.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr int kNone = 1 << 30;                 // not reached so far; every finite cost is below it (the limit on n_out * max_weight)
constexpr int kTileX = 64, kTileY = 8, kTileZ = 8;
constexpr int kRowPitch = kTileX + 2;          // a staged row: halo, 64 cells, halo
constexpr int kRowsY = kTileY + 2;             // staged rows per z, and kTileZ + 2 of those
constexpr int kStaged = (kTileZ + 2) * kRowsY * kRowPitch;
constexpr int kTileRows = kTileZ * kTileY;

struct PlanControl {  // the record the host reads once per round
  unsigned long long changed_tiles, tile_runs;  // sums over all rounds so far
  int32_t seeds_used, pad;
};
constexpr size_t kControlBytes = 32;  // the tile flags of the two rounds follow, then the ring costs
static_assert(sizeof(PlanControl) <= kControlBytes, "the control record, the flags and the ring costs share a slot");

__device__ inline int load_cost(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_cost(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

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

__global__ __launch_bounds__(256) void plan_seed_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, int nx, int ny,
                                                        int nz, int wpr, int tiles_x, int tiles_y,
                                                        const unsigned long long *__restrict__ bits, int32_t *__restrict__ cost,
                                                        int *__restrict__ flags, PlanControl *__restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, y = (long long)seeds[3 * i + 1] - oy, z = (long long)seeds[3 * i + 2] - oz;
  if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) return;
  const long long row = z * ny + y;
  if (!((bits[row * wpr + (x >> 6)] >> (x & 63)) & 1ull)) return;
  store_cost(cost + row * nx + x, 0);
  atomicAdd(&ctl->seeds_used, 1);
  flags[((z / kTileZ) * tiles_y + y / kTileY) * tiles_x + x / kTileX] = 1;
}

// flags_now: this round's (a tile clears its own), flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void plan_relax_kernel(int32_t *__restrict__ cost, const unsigned long long *__restrict__ bits,
                                                         const uint16_t *__restrict__ weights, int nx, int ny, int nz, int wpr, int tiles_x,
                                                         int tiles_y, int tiles_z, int *__restrict__ flags_now, int *__restrict__ flags_next,
                                                         PlanControl *__restrict__ ctl) {
  __shared__ int32_t s[kStaged];
  __shared__ uint16_t wts[kTileRows * kTileX];  // the tile's own cells: row r = z * 8 + y at r * 64
  __shared__ unsigned long long row_bits[kTileRows];
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
    const int32_t *__restrict__ row = cost + ((long long)gz * ny + gy) * nx;
    s[r * kRowPitch + 1 + lane] = row_in && gx < nx ? load_cost(row + gx) : kNone;
    if (lane == 0) s[r * kRowPitch] = row_in && x0 > 0 ? load_cost(row + x0 - 1) : kNone;
    if (lane == 63) s[r * kRowPitch + kTileX + 1] = row_in && x0 + kTileX < nx ? load_cost(row + x0 + kTileX) : kNone;
  }
  for (int r = w; r < kTileRows; r += 4) {
    const int gy = y0 + (r & 7), gz = z0 + (r >> 3);
    wts[r * kTileX + lane] = gy < ny && gz < nz && gx < nx ? weights[((long long)gz * ny + gy) * nx + gx] : (uint16_t)0;
  }
  if (tid < kTileRows) {
    const int gy = y0 + (tid & 7), gz = z0 + (tid >> 3);
    row_bits[tid] = gy < ny && gz < nz ? bits[((long long)gz * ny + gy) * wpr + tx] : 0ull;
  }
  __syncthreads();

  int again;
  do {
    int changed = 0;
    // x: a wavefront per row
    for (int r = w; r < kTileRows; r += 4) {
      const unsigned long long tw = row_bits[r];
      if (tw == 0ull) continue;  // the same for the whole wavefront
      const int at = (((r >> 3) + 1) * kRowsY + (r & 7) + 1) * kRowPitch + 1 + lane;
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
    for (int z = w; z < kTileZ; z += 4) {
      int32_t *col = s + (z + 1) * kRowsY * kRowPitch + 1 + lane;  // the halo cell below the column; the one above is 9 rows on
      const uint16_t *cw = wts + z * kTileY * kTileX + lane;
      changed |= sweep_column_weighted<kNone, kRowPitch, 1, kTileX, true>(col + kRowPitch, row_bits + z * 8, cw, lane, col[0]);
      changed |= sweep_column_weighted<kNone, kRowPitch, 1, kTileX, false>(col + kRowPitch, row_bits + z * 8, cw, lane,
                                                                           col[(kTileY + 1) * kRowPitch]);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileY; y += 4) {
      constexpr int kPlane = kRowsY * kRowPitch;
      int32_t *col = s + (y + 1) * kRowPitch + 1 + lane;
      const uint16_t *cw = wts + y * kTileX + lane;
      changed |= sweep_column_weighted<kNone, kPlane, 8, kTileY * kTileX, true>(col + kPlane, row_bits + y, cw, lane, col[0]);
      changed |= sweep_column_weighted<kNone, kPlane, 8, kTileY * kTileX, false>(col + kPlane, row_bits + y, cw, lane,
                                                                                 col[(kTileZ + 1) * kPlane]);
    }
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  // write back what fell; which faces towards an existing neighbour tile fell
  int mine = 0;
  for (int r = w; r < kTileRows; r += 4) {
    const int y = r & 7, z = r >> 3;
    if (!((row_bits[r] >> lane) & 1ull)) continue;  // a set bit: the cell is inside the region
    const int v = s[((z + 1) * kRowsY + y + 1) * kRowPitch + 1 + lane];
    int32_t *p = cost + ((long long)(z0 + z) * ny + (y0 + y)) * nx + gx;
    if (v < load_cost(p)) {
      store_cost(p, v);
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

__global__ __launch_bounds__(256) void plan_finish_kernel(int32_t *__restrict__ cost, int nx, int wpr, long long words,
                                                          const unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  if (x >= nx) return;
  const long long at = (word / wpr) * nx + x;
  const int v = cost[at];
  cost[at] = !((bits[word] >> lane) & 1ull) ? -2 : v == kNone ? -1 : v;
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
  const long long nx = own.nx, ny = own.ny, nz = own.nz, wpr = own.wpr, words = own.words;
  const long long tiles_x = wpr, tiles_y = (ny + kTileY - 1) / kTileY, tiles_z = (nz + kTileZ - 1) / kTileZ;
  const long long tiles = tiles_x * tiles_y * tiles_z;
  // decided here, before anything is allocated or written: a launch takes at most 2^32 - 1 work-items, and every finite cost has
  // to stay below "none" -- a path has fewer cells than the region, each at most max_weight
  if (own.n_out <= INT_MAX && tiles * 256 > 0xFFFFFFFFll) {
    set_last_error_text("svoslam_pool_cost_field: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)", nx, ny,
                        nz, tiles);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
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
  PlanControl *ctl = ws->plan_ctl.as<PlanControl>();
  int *flags = reinterpret_cast<int *>(ws->plan_ctl.as<char>() + kControlBytes);
  int32_t *ring = reinterpret_cast<int32_t *>(ws->plan_ctl.as<char>() + kControlBytes + flag_bytes);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + flag_bytes, stream));
  if (rings > 0) SVO_HIP(hipMemcpyAsync(ring, h_ring_cost, (size_t)rings * 4, hipMemcpyHostToDevice, stream));
  plan_weigh_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_cost, (int)nx, (int)wpr, words, r, R, ring, bits, weights);
  SVO_LAUNCH_CHECK();  // d_cost has become the working array in place
  if (n_seeds > 0) {
    plan_seed_kernel<<<cdiv(n_seeds, 256), 256, 0, stream>>>(d_seeds, n_seeds, origin[0], origin[1], origin[2], (int)nx, (int)ny, (int)nz,
                                                             (int)wpr, (int)tiles_x, (int)tiles_y, bits, d_cost, flags, ctl);
    SVO_LAUNCH_CHECK();
  }
  // rounds: a round in which no tile lowered anything is the last.  After round k every cell with a cheapest path that crosses at
  // most k tile faces is final, and a path has fewer cells than the region, so the cap below is never reached; it keeps the loop
  // from spinning whatever happens.
  const long long cap = tiles * (long long)(kTileX * kTileY * kTileZ) + 1;
  PlanControl seen = {};
  unsigned long long changed_before = 0;
  long long rounds = 0;
  for (;;) {
    if (rounds >= cap) {
      set_last_error_text("svoslam_pool_cost_field: no convergence after %lld rounds over %lld tiles", rounds, tiles);
      return SVOSLAM_ERR_HIP;
    }
    int *now = flags + (rounds & 1) * tiles, *next = flags + ((rounds + 1) & 1) * tiles;
    plan_relax_kernel<<<(unsigned)tiles, 256, 0, stream>>>(d_cost, bits, weights, (int)nx, (int)ny, (int)nz, (int)wpr, (int)tiles_x,
                                                           (int)tiles_y, (int)tiles_z, now, next, ctl);
    SVO_LAUNCH_CHECK();
    rounds++;
    SVO_HIP(hipMemcpyAsync(&seen, ctl, sizeof(seen), hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    if (seen.changed_tiles == changed_before) break;
    changed_before = seen.changed_tiles;
  }
  plan_finish_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_cost, (int)nx, (int)wpr, words, bits);
  SVO_LAUNCH_CHECK();
  if (stats) {
    stats->rounds = (int32_t)(rounds < INT_MAX ? rounds : INT_MAX);
    stats->tile_runs = (int32_t)(seen.tile_runs < (unsigned long long)INT_MAX ? seen.tile_runs : (unsigned long long)INT_MAX);
    stats->seeds_used = seen.seeds_used;
  }
  return SVOSLAM_OK;
}

int field_trace_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], const int32_t *d_starts, int32_t n_starts,
                      int32_t max_cells, int32_t *d_paths, int32_t *d_lengths, hipStream_t stream) {
  if (!origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n_starts < 0 || max_cells < 0) return SVOSLAM_ERR_INVALID_ARG;
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  const long long plane = empty ? 0 : (long long)dims[0] * dims[1];  // below 2^62; the third factor only after it was tested
  const long long cells = plane > INT_MAX ? plane : plane * dims[2];
  if (cells > INT_MAX) {
    set_last_error_text("svoslam_field_trace_paths: %d x %d x %d cells are more than 2^31 - 1", dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if ((long long)n_starts * max_cells > INT_MAX / 3) {
    set_last_error_text("svoslam_field_trace_paths: %d starts of %d cells are more than 2^31 - 1 path entries", n_starts, max_cells);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_starts == 0) return SVOSLAM_OK;
  if (!d_starts || !d_lengths || (cells > 0 && !d_field) || (max_cells > 0 && !d_paths)) return SVOSLAM_ERR_INVALID_ARG;
  StageScope timed(kStageQuery, stream);
  trace_paths_kernel<<<cdiv(n_starts, 256), 256, 0, stream>>>(d_field, origin[0], origin[1], origin[2], dims[0], dims[1], dims[2], d_starts,
                                                              n_starts, max_cells, d_paths, d_lengths);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
