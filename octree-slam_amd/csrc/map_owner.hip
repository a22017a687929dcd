// map_owner.hip -- the owner field of a map region: the reach field's steps and, for every reached cell, the smallest label among
// the seeds whose shortest path to it has exactly that many moves (own specification, include/svoslam.h and DESIGN.md section 26:
// the reference has nothing like it; the restatement the device must equal value for value is tests/test_owner_cpu.py).  Two
// relaxations of 32-bit values on map_relax.hpp's scheme, d_steps and d_owner their working arrays, the reach slots for T's row
// words, the control record and the flags (with one more int per tile: the tiles the seeds wake):
//
//   phase 1             map_reach.hip's reach_relax: the distance field, the pack, THIS FILE'S SEEDING, the rounds of
//                       reach_relax_kernel on d_steps, the finish (-1 no path, -2 not in T).
//     list form         relax_seed_kernel (steps = 0, the count), owner_fill_kernel (owner = "none" = INT_MAX) and
//                       owner_seed_list_kernel: one atomicMin(&owner[cell], k) per counted entry k.
//     field form        owner_seed_field_kernel: a wavefront per row word, a lane per cell; the lane reads its own label before it
//                       writes steps = 0 and owner = label, or owner = "none": d_seed_field may be d_owner.
//                       Both mark the seed's tile AND the tile across every tile face the seed lies on (relax_mark_seed): a seed's
//                       own values are never "lowered", so the write-back alone would not wake the tile that sees it in its halo.
//   phase 2             owner_relax_kernel, rounds from the marked tiles: owners AND the finished steps staged in LDS (2 x 26400
//                       bytes); owner[q] falls to min(owner[q], owner[p]) over the face neighbours p with steps[p] == steps[q] - 1,
//                       where steps[q] >= 1.  A blocked, unreached or outside cell has steps < 0 and never matches.
//                         x  a wavefront per row: the links steps[x] == steps[x -+ 1] + 1 as two ballots, then owner_sweep_row's
//                            segmented minimum scans by doubling along the chains of links, after the two halo cells;
//                         y, z  owner_sweep_column: a lane per column, serial up and down the 8 cells from the halo.
//                       Passes repeat until one lowers nothing; relax_store_faces writes back what fell and raises the flags.
//   owner_finish_kernel owner = steps where steps < 0.
// Owners only fall, every value an owner takes is the label of a nearest seed, and at the fixed point every cell has taken the
// minimum over all its predecessors: the specified value, whatever the order of workgroups (section 26).
// No cooperative launch, no workgroup waits on another, no persistent kernel, no inline assembly, no per-lane array indexed at run
// time; every device loop ends by its own data; the global accesses of owner_relax_kernel are relaxed agent-scope atomics.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): owner_relax_kernel 69 VGPRs, 88 SGPRs, 53576 bytes of
// static LDS (3 workgroups per CU of 160 KB: occupancy 3, by LDS), 0 bytes of scratch; owner_seed_list_kernel 16 VGPRs, 25 SGPRs;
// owner_seed_field_kernel 15 and 30; owner_fill_kernel 3 and 12; owner_finish_kernel 4 and 12; those four no LDS, occupancy 8, 0
// bytes of scratch.
#include <limits.h>

#include "map_owner.hpp"
#include "map_reach.hpp"
#include "map_relax.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr int kNoOwner = INT_MAX;  // above every label: 0 .. 2^31 - 2
constexpr int kOutside = -2;       // the staged steps of a cell outside the region: as a blocked cell, it never matches

__global__ __launch_bounds__(256) void owner_fill_kernel(int32_t *__restrict__ owner, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i < n) owner[i] = kNoOwner;
}

// relax_seed_kernel's test of an entry; the label of entry i is i
__global__ __launch_bounds__(256) void owner_seed_list_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, TileGrid g,
                                                              const unsigned long long *__restrict__ bits, int32_t *__restrict__ owner,
                                                              int *__restrict__ marks) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, a = (long long)seeds[3 * i + 1] - oy, b = (long long)seeds[3 * i + 2] - oz;
  if (x < 0 || x >= g.nx || a < 0 || a >= g.na || b < 0 || b >= g.nb) return;
  if (!((bits[(a * g.ba + b * g.bb) * g.wpr + (x >> 6)] >> (x & 63)) & 1ull)) return;
  atomicMin(owner + a * g.sa + b * g.sb + x, i);
  relax_mark_seed(marks, g, (int)x, (int)a, (int)b, (x & 63) == 0, (x & 63) == 63);
}

// one wavefront per row word.  seed_field may be owner: no __restrict__ on the two, and each lane reads its cell before it writes it
__global__ __launch_bounds__(256) void owner_seed_field_kernel(const int32_t *seed_field, long long words, TileGrid g,
                                                               const unsigned long long *__restrict__ bits, int32_t *__restrict__ steps,
                                                               int32_t *owner, int *__restrict__ marks, RelaxControl *__restrict__ ctl) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int tx = (int)(word % g.wpr);
  const long long row = word / g.wpr;
  const int x = tx * 64 + lane;
  const bool in = x < g.nx;
  const long long at = row * g.nx + x;
  const int v = in ? seed_field[at] : -1;
  const bool is_seed = in && ((bits[word] >> lane) & 1ull) && v >= 0 && v < kNoOwner;
  if (in) owner[at] = is_seed ? v : kNoOwner;
  if (is_seed) store_value(steps + at, 0);
  const unsigned long long m = __ballot(is_seed);
  if (m != 0ull && lane == 0) {
    atomicAdd(&ctl->seeds_used, __popcll(m));
    relax_mark_seed(marks, g, tx * 64, (int)(row % g.na), (int)(row / g.na), (m & 1ull) != 0ull, (m >> 63) != 0ull);
  }
}

__global__ __launch_bounds__(256) void owner_finish_kernel(int32_t *__restrict__ owner, const int32_t *__restrict__ steps, long long n) {
  const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = steps[i];
  if (s < 0) owner[i] = s;
}

// relax_stage for two arrays: the owners ("none" outside the region) and the finished steps (kOutside there), and the 64 row words
__device__ __forceinline__ void owner_stage(int32_t *__restrict__ so, int32_t *__restrict__ ss, unsigned long long *__restrict__ row_bits,
                                            const int32_t *__restrict__ owner, const int32_t *__restrict__ steps,
                                            const unsigned long long *__restrict__ bits, const TileGrid &g, const TileAt &t) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int gx = t.x0 + lane;
  for (int r = w; r < (kTileB + 2) * kRowsA; r += 4) {
    const int pa = r % kRowsA, pb = r / kRowsA;
    const int ga = t.a0 + pa - 1, gb = t.b0 + pb - 1;
    const bool row_in = ga >= 0 && ga < g.na && gb >= 0 && gb < g.nb;
    const long long row = (long long)ga * g.sa + (long long)gb * g.sb;
    const bool in = row_in && gx < g.nx;
    so[r * kRowPitch + 1 + lane] = in ? load_value(owner + row + gx) : kNoOwner;
    ss[r * kRowPitch + 1 + lane] = in ? load_value(steps + row + gx) : kOutside;
    if (lane == 0) {
      const bool lo = row_in && t.x0 > 0;
      so[r * kRowPitch] = lo ? load_value(owner + row + t.x0 - 1) : kNoOwner;
      ss[r * kRowPitch] = lo ? load_value(steps + row + t.x0 - 1) : kOutside;
    }
    if (lane == 63) {
      const bool hi = row_in && t.x0 + kTileX < g.nx;
      so[r * kRowPitch + kTileX + 1] = hi ? load_value(owner + row + t.x0 + kTileX) : kNoOwner;
      ss[r * kRowPitch + kTileX + 1] = hi ? load_value(steps + row + t.x0 + kTileX) : kOutside;
    }
  }
  if (tid < kTileRows) {
    const int ga = t.a0 + (tid & 7), gb = t.b0 + (tid >> 3);
    row_bits[tid] = ga < g.na && gb < g.nb ? bits[((long long)ga * g.ba + (long long)gb * g.bb) * g.wpr + t.tx] : 0ull;
  }
}

// x: a wavefront per row, a lane per cell, o the cell's owner.  Bit x of `up` : the owner of cell x - 1 may flow to cell x (steps[x]
// == steps[x - 1] + 1); bit x of `down`: that of cell x + 1 may.  Segmented minimum scans by doubling, sweep_row's form: a step of k
// is taken only where all k links between source and target are set, so after the six steps a cell holds the minimum over the
// whole chain of links that ends in it.
__device__ __forceinline__ int owner_sweep_row(int o, unsigned long long up, unsigned long long down, int lane) {
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from below: the links lane - k + 1 .. lane
    const int u = __shfl_up(o, k);
    const unsigned long long run = ((1ull << k) - 1ull) << (lane >= k ? lane - k + 1 : 0);
    if (lane >= k && (up & run) == run) o = min(o, u);
  }
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from above: the links lane .. lane + k - 1
    const int u = __shfl_down(o, k);
    const unsigned long long run = ((1ull << k) - 1ull) << lane;
    if (lane + k < 64 && (down & run) == run) o = min(o, u);
  }
  return o;
}

// y or z: a lane per column, serial over its 8 cells, upwards or downwards, starting from the halo's owner and steps.  Cell c is at
// owners[c * kPitch] and stepped[c * kPitch].  Returns 1 if an owner was lowered, else 0.
template <int kPitch, bool kUp>
__device__ __forceinline__ int owner_sweep_column(int32_t *owners, const int32_t *stepped, int prev_o, int prev_s) {
  int lowered = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = kUp ? i : 7 - i;
    const int s = stepped[c * kPitch];
    int o = owners[c * kPitch];
    if (s >= 1 && prev_s == s - 1 && prev_o < o) {
      o = prev_o;
      owners[c * kPitch] = o;
      lowered = 1;
    }
    prev_o = o, prev_s = s;
  }
  return lowered;
}

// flags_now: this round's, flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void owner_relax_kernel(int32_t *__restrict__ owner, const int32_t *__restrict__ steps,
                                                          const unsigned long long *__restrict__ bits, TileGrid g, int *__restrict__ flags_now,
                                                          int *__restrict__ flags_next, RelaxControl *__restrict__ ctl) {
  __shared__ int32_t so[(kTileB + 2) * kLayer];
  __shared__ int32_t ss[(kTileB + 2) * kLayer];
  __shared__ unsigned long long row_bits[kTileRows];
  __shared__ TileShared sh;
  if (!relax_enter(sh, flags_now)) return;
  const TileAt t = tile_at(g);
  owner_stage(so, ss, row_bits, owner, steps, bits, g, t);
  __syncthreads();

  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  int again;
  do {
    int changed = 0;
    // x: a wavefront per row
    for (int r = w; r < kTileRows; r += 4) {
      if (row_bits[r] == 0ull) continue;  // the same for the whole wavefront
      const int at = staged_at(r & 7, r >> 3, 1) + lane;
      const int s = ss[at], before = so[at];
      int o = before;
      if (lane == 0 && s >= 1 && ss[at - 1] == s - 1) o = min(o, so[at - 1]);
      if (lane == 63 && s >= 1 && ss[at + 1] == s - 1) o = min(o, so[at + 1]);
      const int below = __shfl_up(s, 1), above = __shfl_down(s, 1);
      const unsigned long long up = __ballot(lane >= 1 && s >= 1 && below == s - 1);
      const unsigned long long down = __ballot(lane < 63 && s >= 1 && above == s - 1);
      o = owner_sweep_row(o, up, down, lane);
      if (o < before) { so[at] = o; changed = 1; }
    }
    __syncthreads();
    // y: a lane per (x, z) column
    for (int z = w; z < kTileB; z += 4) {
      const int col = (z + 1) * kLayer + 1 + lane;  // the halo cell below the column; the one above is 9 rows on
      changed |= owner_sweep_column<kRowPitch, true>(so + col + kRowPitch, ss + col + kRowPitch, so[col], ss[col]);
      changed |= owner_sweep_column<kRowPitch, false>(so + col + kRowPitch, ss + col + kRowPitch, so[col + (kTileA + 1) * kRowPitch],
                                                      ss[col + (kTileA + 1) * kRowPitch]);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileA; y += 4) {
      const int col = (y + 1) * kRowPitch + 1 + lane;
      changed |= owner_sweep_column<kLayer, true>(so + col + kLayer, ss + col + kLayer, so[col], ss[col]);
      changed |= owner_sweep_column<kLayer, false>(so + col + kLayer, ss + col + kLayer, so[col + (kTileB + 1) * kLayer],
                                                   ss[col + (kTileB + 1) * kLayer]);
    }
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  relax_store_faces(owner, so, row_bits, sh, g, t, flags_next, ctl);
}

}  // namespace

int pool_owner_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t r, const int32_t *d_seeds, int32_t n_seeds, const int32_t *d_seed_field, int32_t *d_steps,
                     int32_t *d_owner, svoslam_owner_stats *stats, hipStream_t stream) {
  const char *fn = "svoslam_pool_owner_field";
  if (stats) *stats = {};
  if (!ws || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || n_seeds < 0 || (n_seeds > 0 && !d_seeds)) return SVOSLAM_ERR_INVALID_ARG;
  if (d_seed_field && (d_seeds || n_seeds != 0)) return SVOSLAM_ERR_INVALID_ARG;  // one seed form
  RegionPlan own;
  SVO_TRY(plan_region(depth, origin, dims, 0, &own));
  if (own.nothing) return SVOSLAM_OK;
  if (!d_steps || !d_owner || d_steps == d_owner) return SVOSLAM_ERR_INVALID_ARG;

  AdoptedBracket bracket(stream);  // one bracket, around both phases
  ReachFrame f;
  long long rounds, owner_rounds;
  RelaxControl seen, owner_seen;
  SVO_TRY(reach_relax(fn, ws, pool, depth, origin, dims, r, d_steps, 1, [&](const ReachFrame &fr) -> int {
    int *marks = fr.flags + 2 * fr.tiles;  // the tiles the seeds wake: round 0's flags of both phases
    SVO_HIP(hipMemsetAsync(marks, 0, (size_t)fr.tiles * 4, stream));
    if (d_seed_field) {
      owner_seed_field_kernel<<<cdiv(fr.own.words, 4), 256, 0, stream>>>(d_seed_field, fr.own.words, fr.g, fr.bits, d_steps, d_owner, marks,
                                                                        fr.ctl);
      SVO_LAUNCH_CHECK();
    } else {
      SVO_TRY(relax_seed(d_seeds, n_seeds, origin, fr.g, fr.bits, d_steps, fr.flags, fr.ctl, stream));
      owner_fill_kernel<<<cdiv(fr.own.n_out, 256), 256, 0, stream>>>(d_owner, fr.own.n_out);
      SVO_LAUNCH_CHECK();
      if (n_seeds > 0) {
        owner_seed_list_kernel<<<cdiv(n_seeds, 256), 256, 0, stream>>>(d_seeds, n_seeds, origin[0], origin[1], origin[2], fr.g, fr.bits,
                                                                       d_owner, marks);
        SVO_LAUNCH_CHECK();
      }
    }
    SVO_HIP(hipMemcpyAsync(fr.flags, marks, (size_t)fr.tiles * 4, hipMemcpyDeviceToDevice, stream));
    return SVOSLAM_OK;
  }, bracket, &f, &rounds, &seen, stream));

  // phase 2, on the finished steps: the control record and the flags start again, from the same tiles
  SVO_HIP(hipMemsetAsync(f.ctl, 0, kControlBytes + (size_t)f.tiles * 8, stream));
  SVO_HIP(hipMemcpyAsync(f.flags, f.flags + 2 * f.tiles, (size_t)f.tiles * 4, hipMemcpyDeviceToDevice, stream));
  const TileGrid g = f.g;
  SVO_TRY(relax_rounds(fn, f.tiles, f.ctl, f.flags, stream, [&](int *now, int *next) {
    owner_relax_kernel<<<(unsigned)f.tiles, 256, 0, stream>>>(d_owner, d_steps, f.bits, g, now, next, f.ctl);
  }, &owner_rounds, &owner_seen));
  owner_finish_kernel<<<cdiv(f.own.n_out, 256), 256, 0, stream>>>(d_owner, d_steps, f.own.n_out);
  SVO_LAUNCH_CHECK();
  if (stats) {
    svoslam_reach_stats a, b;
    relax_stats(&a, rounds, seen);
    relax_stats(&b, owner_rounds, owner_seen);
    stats->rounds = a.rounds, stats->tile_runs = a.tile_runs, stats->seeds_used = a.seeds_used;
    stats->owner_rounds = b.rounds, stats->owner_tile_runs = b.tile_runs;
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
