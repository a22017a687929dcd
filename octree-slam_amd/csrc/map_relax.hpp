// map_relax.hpp -- the tiled relaxation behind the reach field (map_reach.hip), the cost field (map_plan.hip) and the ground field
// (map_ground.hip): DESIGN.md section 16.  A field of 32-bit values over a region, "none" (2^30) where nothing has arrived, is lowered
// towards its unique fixed point by rounds of one launch each:
//
//   one workgroup of 256 per tile of 64 x 8 x 8 cells (x and two other axes, a and b: y and z, or ground's h and t), launched over
//   all tiles; a tile whose flag of this round is clear leaves at once (relax_enter).  The tile's values are staged in LDS with a
//   halo of one cell on x and a and of `halo` cells on b, rows of 66 dwords, with its 64 row words (relax_stage); outside the
//   region the halo is "none".  The caller's passes lower the staged values until one changes nothing.  Then every lane compares
//   its cells with global memory and stores the lowered ones (relax_store); a rule of the caller's says which neighbour tiles see
//   a lowered cell in their halo, and next round's flags of those are raised, with the counter of changed tiles (relax_store_faces:
//   reach and cost; ground has its own rule).  Other workgroups read those cells as their halo during the same
//   launch: all global accesses to the values are relaxed 32-bit agent-scope atomics.  Whichever value a neighbour saw, it runs
//   again next round if a cell it sees fell, and values only fall.
//
//   The host (relax_rounds) launches rounds until the counter of changed tiles stands still, reading 32 bytes per round: the call
//   blocks.  No cooperative launch, no workgroup waits on another, every device loop ends by its own data, the rounds are capped.
//
// map_relax.hip holds what is the same kernel for every field -- relax_seed_kernel (reach and cost) and relax_finish_kernel -- and
// the host checks that differ by the public function's name only.  It opens no kStageQuery bracket: its callers do.
#pragma once
#include <limits.h>

#include "common.hpp"

namespace svoslam {

constexpr int kNone = 1 << 30;                   // not reached so far; every finite value is below it, and kNone + 2^22 fits an int32
constexpr int kTileX = 64, kTileA = 8, kTileB = 8;
constexpr int kRowPitch = kTileX + 2;            // a staged row: halo, 64 cells, halo
constexpr int kRowsA = kTileA + 2;               // staged rows per layer of b
constexpr int kLayer = kRowsA * kRowPitch;       // and kTileB + 2 * halo of those layers
constexpr int kTileRows = kTileB * kTileA;       // row r = b * 8 + a of the tile's own cells

struct RelaxControl {  // the record the host reads once per round
  unsigned long long changed_tiles, tile_runs;  // sums over all rounds so far
  int32_t seeds_used, footholds;                // footholds: the ground field's alone
};
constexpr size_t kControlBytes = 32;  // the tile flags of the two rounds follow in the same slot
static_assert(sizeof(RelaxControl) <= kControlBytes, "the control record and the flags share a slot");

struct TileGrid {    // a region as x and two other axes a and b, cut into tiles
  int nx, na, nb;    // cells per axis
  int sa, sb;        // strides of a and b in the value array: a region has at most 2^31 - 1 cells
  int ba, bb;        // strides of a and b in the region's bit rows
  int wpr;           // 64-bit words per bit row
  int tiles_x, tiles_a, tiles_b;
  long long tiles() const { return (long long)tiles_x * tiles_a * tiles_b; }
};

inline TileGrid tile_grid(long long nx, long long na, long long nb, long long sa, long long sb, long long ba, long long bb, long long wpr) {
  TileGrid g;
  g.nx = (int)nx, g.na = (int)na, g.nb = (int)nb, g.sa = (int)sa, g.sb = (int)sb, g.ba = (int)ba, g.bb = (int)bb, g.wpr = (int)wpr;
  g.tiles_x = (int)wpr, g.tiles_a = (int)((na + kTileA - 1) / kTileA), g.tiles_b = (int)((nb + kTileB - 1) / kTileB);
  return g;
}

// ---- host (map_relax.hip) --------------------------------------------------------------------------------------------------------

// a launch takes at most 2^32 - 1 work-items: SVOSLAM_ERR_POOL_LIMIT, worded for the public function `fn` and the region's nx x ny
// x nz cells, when the grid has more tiles than that
int relax_tile_limit(const char *fn, const TileGrid &g, long long ny, long long nz);
// one lane per seed entry (x, y, z; the grid's a = y, b = z): a seed in the region whose bit is set writes 0, is counted, and marks
// its tile and the tiles that see it in their halo (relax_mark_seed)
int relax_seed(const int32_t *d_seeds, int n_seeds, const int32_t origin[3], const TileGrid &g, const unsigned long long *bits,
               int32_t *values, int *flags, RelaxControl *ctl, hipStream_t stream);
// "none" becomes -1, a cell without its bit -2
int relax_finish(int32_t *values, long long nx, long long wpr, long long words, const unsigned long long *bits, hipStream_t stream);
// the argument and limit checks of a trace function, worded for `fn`; *launch: there are starts to trace
int trace_arguments(const char *fn, const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], const int32_t *d_starts,
                    int32_t n_starts, int32_t max_cells, const int32_t *d_paths, const int32_t *d_lengths, bool *launch);

// rounds: launch(now, next) enqueues one round over the flags of this round and of the coming one.  A round in which no tile
// lowered anything is the last.  After round k every cell with a cheapest path that leaves a tile at most k times is final, and a
// path has fewer cells than the region, so the cap is never reached; it keeps the loop from spinning whatever happens.
template <class Launch>
int relax_rounds(const char *fn, long long tiles, const RelaxControl *ctl, int *flags, hipStream_t stream, Launch launch,
                 long long *rounds, RelaxControl *seen) {
  const long long cap = tiles * (long long)(kTileX * kTileA * kTileB) + 1;
  unsigned long long changed_before = 0;
  *seen = {};
  for (*rounds = 0;;) {
    if (*rounds >= cap) {
      set_last_error_text("%s: no convergence after %lld rounds over %lld tiles", fn, *rounds, tiles);
      return SVOSLAM_ERR_HIP;
    }
    launch(flags + (*rounds & 1) * tiles, flags + ((*rounds + 1) & 1) * tiles);
    SVO_LAUNCH_CHECK();
    ++*rounds;
    SVO_HIP(hipMemcpyAsync(seen, ctl, sizeof(*seen), hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    if (seen->changed_tiles == changed_before) return SVOSLAM_OK;
    changed_before = seen->changed_tiles;
  }
}

template <class Stats>
void relax_stats(Stats *stats, long long rounds, const RelaxControl &seen) {
  stats->rounds = (int32_t)(rounds < INT_MAX ? rounds : INT_MAX);
  stats->tile_runs = (int32_t)(seen.tile_runs < (unsigned long long)INT_MAX ? seen.tile_runs : (unsigned long long)INT_MAX);
  stats->seeds_used = seen.seeds_used;
}

// ---- device ----------------------------------------------------------------------------------------------------------------------

__device__ inline int load_value(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_value(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

struct TileShared {  // a relax kernel's static LDS beside the staged values and the kTileRows row words
  int go, faces;
};

struct TileAt {  // the workgroup's tile: its index, its place in the grid and its first cell
  int tile, tx, ta, tb, x0, a0, b0;
};

// flags_now: this round's (a tile clears its own).  False: the flag was clear and the whole workgroup leaves
__device__ __forceinline__ bool relax_enter(TileShared &sh, int *__restrict__ flags_now) {
  if (threadIdx.x == 0) {
    const unsigned tile = blockIdx.x;
    sh.go = flags_now[tile];
    flags_now[tile] = 0;
    sh.faces = 0;
  }
  __syncthreads();
  return sh.go != 0;
}

__device__ __forceinline__ TileAt tile_at(const TileGrid &g) {
  TileAt t;
  t.tile = blockIdx.x;
  t.tx = t.tile % g.tiles_x, t.ta = (t.tile / g.tiles_x) % g.tiles_a, t.tb = t.tile / (g.tiles_x * g.tiles_a);
  t.x0 = t.tx * kTileX, t.a0 = t.ta * kTileA, t.b0 = t.tb * kTileB;
  return t;
}

// the cell (x, a, b) of the tile is at dword staged_at(a, b, halo) + x of the staged values
__device__ __forceinline__ int staged_at(int a, int b, int halo) { return ((b + halo) * kRowsA + a + 1) * kRowPitch + 1; }

// staged row r = pb * 10 + pa of s is the row a0 + pa - 1, b0 + pb - halo of the region; outside the region: "none".  With the 64
// row words.  No barrier: the caller's comes after whatever else it stages
__device__ __forceinline__ void relax_stage(int32_t *__restrict__ s, unsigned long long *__restrict__ row_bits,
                                            const int32_t *__restrict__ values, const unsigned long long *__restrict__ bits,
                                            const TileGrid &g, const TileAt &t, int halo) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gx = t.x0 + lane;
  for (int r = w; r < (kTileB + 2 * halo) * kRowsA; r += 4) {
    const int pa = r % kRowsA, pb = r / kRowsA;
    const int ga = t.a0 + pa - 1, gb = t.b0 + pb - halo;
    const bool row_in = ga >= 0 && ga < g.na && gb >= 0 && gb < g.nb;
    const int32_t *__restrict__ row = values + ((long long)ga * g.sa + (long long)gb * g.sb);
    s[r * kRowPitch + 1 + lane] = row_in && gx < g.nx ? load_value(row + gx) : kNone;
    if (lane == 0) s[r * kRowPitch] = row_in && t.x0 > 0 ? load_value(row + t.x0 - 1) : kNone;
    if (lane == 63) s[r * kRowPitch + kTileX + 1] = row_in && t.x0 + kTileX < g.nx ? load_value(row + t.x0 + kTileX) : kNone;
  }
  if (tid < kTileRows) {
    const int ga = t.a0 + (tid & 7), gb = t.b0 + (tid >> 3);
    row_bits[tid] = ga < g.na && gb < g.nb ? bits[((long long)ga * g.ba + (long long)gb * g.bb) * g.wpr + t.tx] : 0ull;
  }
}

// write back what fell.  seen_by(lane, a, b): a bit per neighbour tile that holds the cell in its halo, for the caller to raise the
// flags by; `any` is added for every lowered cell.  Returns the OR over the workgroup, behind a barrier
template <class Rule>
__device__ __forceinline__ int relax_store(int32_t *__restrict__ values, const int32_t *__restrict__ s,
                                           const unsigned long long *__restrict__ row_bits, TileShared &sh, const TileGrid &g,
                                           const TileAt &t, int halo, int any, Rule seen_by) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int mine = 0;
  for (int r = w; r < kTileRows; r += 4) {
    const int a = r & 7, b = r >> 3;
    if (!((row_bits[r] >> lane) & 1ull)) continue;  // a set bit: the cell is inside the region
    const int v = s[staged_at(a, b, halo) + lane];
    int32_t *p = values + ((long long)(t.a0 + a) * g.sa + (long long)(t.b0 + b) * g.sb + t.x0 + lane);
    if (v < load_value(p)) {
      store_value(p, v);
      mine |= any | seen_by(lane, a, b);
    }
  }
  if (mine) atomicOr(&sh.faces, mine);
  __syncthreads();
  return sh.faces;
}

// f: relax_store's result.  The tile ran; it counts as changed if it lowered anything
__device__ __forceinline__ void relax_count(int f, RelaxControl *__restrict__ ctl) {
  if (threadIdx.x == 0) {
    if (f) atomicAdd(&ctl->changed_tiles, 1ull);
    atomicAdd(&ctl->tile_runs, 1ull);
  }
}

// Round 0's flags of a seed at cell (x, a, b) of a field whose moves go to face neighbours: its own tile, and the tile across every
// tile face the cell lies on, where there is one (on_lo_x, on_hi_x: the cell is lane 0, lane 63 of its row word).  The write-back
// raises flags for cells that FELL; a seed's own value is in place before the first round and never falls, so without this a seed
// whose in-tile neighbours are all blocked would leave the tile that sees it in its halo asleep.
__device__ __forceinline__ void relax_mark_seed(int *__restrict__ flags, const TileGrid &g, int x, int a, int b, bool on_lo_x, bool on_hi_x) {
  const int tx = x / kTileX, ta = a / kTileA, tb = b / kTileB;
  const int tile = (tb * g.tiles_a + ta) * g.tiles_x + tx;
  flags[tile] = 1;
  if (on_lo_x && tx > 0) flags[tile - 1] = 1;
  if (on_hi_x && tx + 1 < g.tiles_x) flags[tile + 1] = 1;
  if (a % kTileA == 0 && ta > 0) flags[tile - g.tiles_x] = 1;
  if (a % kTileA == kTileA - 1 && ta + 1 < g.tiles_a) flags[tile + g.tiles_x] = 1;
  if (b % kTileB == 0 && tb > 0) flags[tile - g.tiles_x * g.tiles_a] = 1;
  if (b % kTileB == kTileB - 1 && tb + 1 < g.tiles_b) flags[tile + g.tiles_x * g.tiles_a] = 1;
}

// The rule of the fields whose moves go to face neighbours (reach, cost): a lowered cell on a face of the tile is seen by the
// neighbour tile across that face, where there is one.  Bits 0..5: -x +x -a +a -b +b; bit 6: anything fell.
__device__ __forceinline__ void relax_store_faces(int32_t *__restrict__ values, const int32_t *__restrict__ s,
                                                  const unsigned long long *__restrict__ row_bits, TileShared &sh, const TileGrid &g,
                                                  const TileAt &t, int *__restrict__ flags_next, RelaxControl *__restrict__ ctl) {
  const int f = relax_store(values, s, row_bits, sh, g, t, 1, 64, [&](int lane, int a, int b) {
    int seen = 0;
    if (lane == 0 && t.tx > 0) seen |= 1;
    if (lane == 63 && t.tx + 1 < g.tiles_x) seen |= 2;
    if (a == 0 && t.ta > 0) seen |= 4;
    if (a == kTileA - 1 && t.ta + 1 < g.tiles_a) seen |= 8;
    if (b == 0 && t.tb > 0) seen |= 16;
    if (b == kTileB - 1 && t.tb + 1 < g.tiles_b) seen |= 32;
    return seen;
  });
  if (threadIdx.x == 0) {
    if (f & 1) flags_next[t.tile - 1] = 1;
    if (f & 2) flags_next[t.tile + 1] = 1;
    if (f & 4) flags_next[t.tile - g.tiles_x] = 1;
    if (f & 8) flags_next[t.tile + g.tiles_x] = 1;
    if (f & 16) flags_next[t.tile - g.tiles_x * g.tiles_a] = 1;
    if (f & 32) flags_next[t.tile + g.tiles_x * g.tiles_a] = 1;
  }
  relax_count(f, ctl);
}

}  // namespace svoslam
