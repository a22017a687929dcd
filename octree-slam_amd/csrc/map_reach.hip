// map_reach.hip -- the reach field of a map region: for every cell of a box of cells the number of face-neighbour moves of the
// shortest path from any seed cell through traversable cells of the region, -1 where there is no such path, -2 where the cell is
// not traversable (own specification, DESIGN.md section 16: the reference has nothing like it; the restatement the device must
// equal value for value is tests/test_reach_cpu.py).  A cell is traversable iff svoslam_pool_distance_field with R =
// clearance_cells writes -1 there, so the field is computed first, by the existing host function and its kernels, into d_steps
// itself; everything after it is integers on the region.
//
//   reach_pack_kernel   one wavefront per 64 consecutive x of a row: the ballot of dist2 == -1 is the row word of the traversable
//                       bits (field_raster_kernel's layout, for the region itself), written by lane 0 with one vector store; every
//                       lane then overwrites its own dist2 with "none" (2^30): d_steps becomes the working array in place, and no
//                       slot of the size of the output is needed.
//   reach_seed_kernel   one lane per seed entry: a seed in the region whose bit is set writes 0, is counted, and marks its tile.
//   reach_relax_kernel  one workgroup of 256 per tile of 64 x 8 x 8 cells, launched over all tiles; a tile whose flag of this
//                       round is clear leaves at once.  The tile's steps with a one-cell halo (10 x 10 rows of 66 dwords, 26400
//                       bytes) and its 64 row words are staged in LDS.  One pass = three sweeps, each exact along its axis:
//                         x  a wavefront per row, a lane per cell: min-plus prefix scans up and down the row by doubling (k = 1,
//                            2, .. 32 through __shfl_up / __shfl_down); a step of k is taken only where the row word has all of
//                            the k + 1 bits from source to target set, so nothing passes through a blocked cell;
//                         y  a lane per (x, z) column, serial up and down the 8 cells from the halo, x across the lanes;
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
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): reach_relax_kernel 58 VGPRs, 90 SGPRs, 27176 bytes of
// static LDS (6 workgroups per CU of 160 KB), occupancy 6 by registers; reach_pack_kernel and reach_finish_kernel 14 VGPRs,
// reach_seed_kernel 12, no LDS, occupancy 8; every kernel 0 bytes of scratch.  No per-lane arrays indexed at run time, no inline
// assembly.
#include <limits.h>

#include "map_field.hpp"
#include "map_reach.hpp"
#include "stage_timing.hpp"
#include "workspace.hpp"

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

__global__ __launch_bounds__(256) void reach_pack_kernel(int32_t *__restrict__ steps, int nx, int wpr, long long words,
                                                         unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  const long long at = (word / wpr) * nx + x;
  const bool in = x < nx;
  const unsigned long long row_word = __ballot(in && steps[at] == -1);
  if (in) steps[at] = kNone;
  if (lane == 0) bits[word] = row_word;
}

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
#pragma unroll
      for (int k = 1; k < 64; k *= 2) {  // from below: cells lane - k .. lane all traversable
        const int u = __shfl_up(v, k);
        const unsigned long long run = ((2ull << k) - 1ull) << (lane >= k ? lane - k : 0);
        if (lane >= k && (tw & run) == run) v = min(v, u + k);
      }
#pragma unroll
      for (int k = 1; k < 64; k *= 2) {  // from above: cells lane .. lane + k
        const int u = __shfl_down(v, k);
        const unsigned long long run = ((2ull << k) - 1ull) << lane;
        if (lane + k < 64 && (tw & run) == run) v = min(v, u + k);
      }
      if (v < before) { s[at] = v; changed = 1; }
    }
    __syncthreads();
    // y: a lane per (x, z) column
    for (int z = w; z < kTileZ; z += 4) {
      const int col = (z + 1) * kRowsY * kRowPitch + 1 + lane;
      int prev = s[col];
#pragma unroll
      for (int y = 0; y < kTileY; y++) {
        const int at = col + (y + 1) * kRowPitch, v = s[at];
        if ((row_bits[z * 8 + y] >> lane) & 1ull) {
          prev = min(v, prev + 1);
          if (prev < v) { s[at] = prev; changed = 1; }
        } else {
          prev = kNone;
        }
      }
      prev = s[col + (kTileY + 1) * kRowPitch];
#pragma unroll
      for (int y = kTileY - 1; y >= 0; y--) {
        const int at = col + (y + 1) * kRowPitch, v = s[at];
        if ((row_bits[z * 8 + y] >> lane) & 1ull) {
          prev = min(v, prev + 1);
          if (prev < v) { s[at] = prev; changed = 1; }
        } else {
          prev = kNone;
        }
      }
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileY; y += 4) {
      const int col = (y + 1) * kRowPitch + 1 + lane;
      int prev = s[col];
#pragma unroll
      for (int z = 0; z < kTileZ; z++) {
        const int at = col + (z + 1) * kRowsY * kRowPitch, v = s[at];
        if ((row_bits[z * 8 + y] >> lane) & 1ull) {
          prev = min(v, prev + 1);
          if (prev < v) { s[at] = prev; changed = 1; }
        } else {
          prev = kNone;
        }
      }
      prev = s[col + (kTileZ + 1) * kRowsY * kRowPitch];
#pragma unroll
      for (int z = kTileZ - 1; z >= 0; z--) {
        const int at = col + (z + 1) * kRowsY * kRowPitch, v = s[at];
        if ((row_bits[z * 8 + y] >> lane) & 1ull) {
          prev = min(v, prev + 1);
          if (prev < v) { s[at] = prev; changed = 1; }
        } else {
          prev = kNone;
        }
      }
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
  if (!ws || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_INVALID_ARG;
  if (r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || n_seeds < 0 || (n_seeds > 0 && !d_seeds)) return SVOSLAM_ERR_INVALID_ARG;
  bool nothing = false;
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > (1ll << depth)) return SVOSLAM_ERR_INVALID_ARG;
    nothing = nothing || dims[a] == 0;
  }
  if (nothing) return SVOSLAM_OK;
  const long long nx = dims[0], ny = dims[1], nz = dims[2];
  const long long wpr = (nx + 63) / 64, words = wpr * ny * nz;  // <= the field's own row words: within its limits
  const long long tiles_x = wpr, tiles_y = (ny + kTileY - 1) / kTileY, tiles_z = (nz + kTileZ - 1) / kTileZ;
  const long long tiles = tiles_x * tiles_y * tiles_z;
  // a launch takes at most 2^32 - 1 work-items: decided here, before anything is allocated or written (the products cannot
  // overflow: every side is <= 2^16)
  if ((long long)dims[0] * dims[1] * dims[2] <= INT_MAX && tiles * 256 > 0xFFFFFFFFll) {
    set_last_error_text("svoslam_pool_reach_field: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)", nx,
                        ny, nz, tiles);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  // the traversable set, as the field's -1, in d_steps: the rest of the argument checks, the field's limits (decided before
  // anything is allocated), the drain of pending fusions and the field's own slots are pool_distance_field's
  svoslam::DeviceBuffer *slots[5] = {&ws->field_bits, &ws->field_a, &ws->field_b, &ws->reach_bits, &ws->reach_flags};
  size_t had[5];
  for (int k = 0; k < 5; k++) had[k] = slots[k]->bytes;
  AdoptedBracket bracket(stream);
  SVO_TRY(pool_distance_field(ws, pool, depth, origin, dims, r, d_steps, nullptr, stream, &bracket.token));
  int rc = ws->reach_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->reach_flags.reserve(kControlBytes + (size_t)tiles * 8);
  if (rc != SVOSLAM_OK) {  // the slots this call grew do not stay behind; the field's launches have finished before theirs go
    (void)hipStreamSynchronize(stream);
    for (int k = 0; k < 5; k++)
      if (slots[k]->bytes != had[k]) slots[k]->release();
    return rc;
  }
  unsigned long long *bits = ws->reach_bits.as<unsigned long long>();
  ReachControl *ctl = ws->reach_flags.as<ReachControl>();
  int *flags = reinterpret_cast<int *>(ws->reach_flags.as<char>() + kControlBytes);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + (size_t)tiles * 8, stream));
  reach_pack_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_steps, (int)nx, (int)wpr, words, bits);
  SVO_LAUNCH_CHECK();
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
