// map_ground.hip -- ground navigation in a map region (own specification, DESIGN.md section 23: the reference has nothing like it;
// the restatements the device must equal value for value are in tests/test_ground_cpu.py).
//
// pool_ground_field: the cost-to-go field of a robot that stands on surfaces.  With u the unit vector of `up` (the y or the z axis,
// either sign), r the body radius, H its height, S the largest step and c the price of a cell climbed, a region cell q is a
// foothold iff q - u is an occupied cell of the root, q + k u is free for k < H, and for S <= k < H no occupied cell of the layer of
// q + k u lies within r of it horizontally.  A move goes from a foothold to a foothold one cell away horizontally and at most S
// cells up or down, and costs 1 + c |j|.  The value of a foothold is the cheapest chain of moves from a seed's foothold; -1 without
// one, -2 where the cell is no foothold.  Axes below: x, h (the other horizontal axis) and t (the up axis).
//
//   body bits            the occupancy raster of the region inflated by r horizontally, 1 below and H - 1 above (region_raster), its
//                        planar distance transform with radius r (region_transform_planar: the x pass and the h pass, no pass along
//                        t), packed into bit rows D = "an occupied cell within r in this layer" (region_pack).  At r = 0, D is the
//                        raster itself and the transform is skipped.
//   ground_mask_kernel   one lane per 64-bit row word of the region: G = O(q - u) AND, over k < H, NOT O(q + k u) AND, over S <= k <
//                        H, NOT D(q + k u).  Rows along u are other rows of the same word column: H + 1 word loads of O (two each
//                        where the inflated rows start off a word boundary) and H - S of D, no per-bit work.  A row outside the
//                        inflated range is outside the root and reads as zero.  The popcounts are summed into `footholds`; then
//                        every wavefront fills the 64 cells of its workgroup's words with "none" (2^30), 256 bytes per store.
//   ground_seed_kernel   one lane per seed entry: from the seed against u, at most snap + 1 bits of G, inside the region; the first
//                        set one writes 0, is counted, and marks its tile and every neighbour tile whose halo holds it (the rule of
//                        the relax kernel's flags below): the seed's own tile need not lower anything that would.
//   ground_relax_kernel  section 16's scheme: one workgroup of 256 per tile of 64 x 8 x 8 cells (x, h, t), launched over all tiles, a
//                        tile whose flag of this round is clear leaves at once.  Staged in dynamic LDS: the tile's costs with a halo
//                        of one cell along x and h and S cells along t, (8 + 2 S) * 10 * 66 values (21120 bytes at S = 0, 42240 at S
//                        = 4), and its 64 foothold words.  A horizontal move flips the parity of x + h, so one pass is two
//                        half-passes by that parity with a barrier between: a lane writes only cells of the half-pass's colour and
//                        reads only the other colour (and halo cells, which nobody writes), free of races and deterministic.  Each
//                        wavefront takes the rows h = 2 p and 2 p + 1 of one t together, even lanes on one row and odd lanes on
//                        the other, so that all 64 lanes hold a cell of the colour; their LDS addresses fall on 64 different dwords
//                        with distinct banks per 32-lane half (pitch 66: an even lane x reads bank x, an odd lane x + 66 = x + 2 mod 32).
//                        A cell reads its 4 (2 S + 1) sources; a cell without its bit is skipped and holds "none", which no sum
//                        reaches from below.  Passes repeat until one changes nothing (__syncthreads_or); then the lowered cells
//                        are stored and next round's flags raised: the horizontal face neighbour of a lowered border column; the
//                        tile above or below THAT one when the cell lies within S of the tile's top or bottom; and the tile
//                        straight above or below for any lowered cell within S of the top or bottom -- no move is vertical, but
//                        a move inside the tile's x and h range that climbs across its top lands there.  Up to 14 neighbours.
//                        All global accesses to the costs are relaxed 32-bit agent-scope atomics.
//   ground_finish_kernel "none" becomes -1, a cell without its bit -2.
// The host launches rounds until the counter of changed tiles stands still, reading 32 bytes per round: the call blocks.  No
// cooperative launch, no workgroup waits on another, every device loop ends by its own data, and the rounds are capped.
//
// field_trace_ground_paths: trace_ground_paths_kernel, one lane per start: the start is snapped like a seed (the first value other
// than -2), then from a cell of value v > 0 the walk takes the first candidate q + e + j u with a value v' >= 0 and v' + 1 + c |j|
// == v, e in the order -x +x -h +h and j = 0, -1, +1, -2, +2, ... within one e.  The values fall strictly.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in DESIGN.md section 23.  Every kernel 0 bytes of scratch,
// no per-lane arrays indexed at run time, no inline assembly; every store is a vector store from plain C++.
#include <limits.h>

#include "map_ground.hpp"
#include "map_region.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

typedef unsigned long long u64;

constexpr int kNone = 1 << 30;  // not reached so far; every finite cost is below it (the limit on n_out * (1 + c S))
constexpr int kTileX = 64, kTileH = 8, kTileT = 8;
constexpr int kRowPitch = kTileX + 2;            // a staged row: halo, 64 cells, halo
constexpr int kRowsH = kTileH + 2;               // staged rows per layer of t
constexpr int kLayer = kRowsH * kRowPitch;       // and 8 + 2 S of those layers
constexpr int kTileRows = kTileT * kTileH;

struct GroundControl {  // the record the host reads once per round
  u64 changed_tiles, tile_runs;  // sums over all rounds so far
  int32_t seeds_used, footholds;
};
constexpr size_t kControlBytes = 32;  // the tile flags of the two rounds follow
static_assert(sizeof(GroundControl) <= kControlBytes, "the control record and the flags share a slot");

struct GroundAxes {   // the region seen as x, h (the other horizontal axis) and t (the up axis)
  int nx, nh, nt, ny; // cells per axis; ny decodes a bit row: row = z * ny + y
  int up_axis, sign;  // 1 = y, 2 = z; +1 or -1: u = sign * (unit vector of up_axis)
  long long sh, st;   // strides of h and t in the cost array
  int bh, bt;         // strides of h and t in the region's bit rows
  int wpr;            // 64-bit words per bit row of the region
  int tiles_x, tiles_h, tiles_t;
};

struct BodyRows {     // the rows of the inflated raster O and of the body bits D
  int off_x, off_h, off_t, len_t;  // the region's first cell inside the inflated one; inflated cells along t
  int wpr_o;                       // words per row of O
  int oh, ot, dh, dt;              // row strides of h' and t' in O, of h and t' in D
};

__device__ inline int load_cost(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_cost(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// 64 bits of a row of O from bit 64 * wi + shift on; behind the row's last word: zero
__device__ inline u64 shifted_word(const u64 *__restrict__ row, int wi, int shift, int wpr) {
  u64 v = row[wi] >> shift;
  if (shift && wi + 1 < wpr) v |= row[wi + 1] << (64 - shift);
  return v;
}

__global__ __launch_bounds__(256) void ground_mask_kernel(const u64 *__restrict__ O, const u64 *__restrict__ D, GroundAxes ax, BodyRows b,
                                                          int H, int S, long long words, u64 *__restrict__ G,
                                                          int32_t *__restrict__ cost, GroundControl *__restrict__ ctl) {
  const long long word = (long long)blockIdx.x * 256 + threadIdx.x;
  if (word < words) {
    const int wx = (int)(word % ax.wpr);
    const long long row = word / ax.wpr;
    const int q = (int)(row / ax.ny), rm = (int)(row % ax.ny);
    const int h = ax.up_axis == 1 ? q : rm, t = ax.up_axis == 1 ? rm : q;
    const long long ho = (long long)(h + b.off_h) * b.oh, hd = (long long)h * b.dh;
    const int ti = t + b.off_t, wi = wx + (b.off_x >> 6), shift = b.off_x & 63;
    u64 g = 0ull;
    const int under = ti - ax.sign;
    if (under >= 0 && under < b.len_t) {  // else q - u is no cell of the root
      g = shifted_word(O + (ho + (long long)under * b.ot) * b.wpr_o, wi, shift, b.wpr_o);
      for (int k = 0; k < H && g; k++) {
        const int tk = ti + ax.sign * k;
        if (tk < 0 || tk >= b.len_t) break;  // through the root's face: nothing is occupied from here on
        g &= ~shifted_word(O + (ho + (long long)tk * b.ot) * b.wpr_o, wi, shift, b.wpr_o);
        if (k >= S) g &= ~D[(hd + (long long)tk * b.dt) * ax.wpr + wx];
      }
    }
    if (wx == ax.wpr - 1 && (ax.nx & 63)) g &= (1ull << (ax.nx & 63)) - 1ull;  // bits behind the region's last x
    G[word] = g;
    if (g) atomicAdd(&ctl->footholds, __popcll(g));
  }
  // the cells of this workgroup's 256 words become "none": a wavefront per word, 64 consecutive values per store
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < 256; i += 4) {
    const long long wd = (long long)blockIdx.x * 256 + i;
    if (wd >= words) break;
    const int x = (int)(wd % ax.wpr) * 64 + lane;
    if (x < ax.nx) cost[(wd / ax.wpr) * ax.nx + x] = kNone;
  }
}

__global__ __launch_bounds__(256) void ground_seed_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, GroundAxes ax,
                                                          int S, int snap, const u64 *__restrict__ G, int32_t *__restrict__ cost,
                                                          int *__restrict__ flags, GroundControl *__restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, y = (long long)seeds[3 * i + 1] - oy, z = (long long)seeds[3 * i + 2] - oz;
  const long long h = ax.up_axis == 1 ? z : y, t0 = ax.up_axis == 1 ? y : z;
  if (x < 0 || x >= ax.nx || h < 0 || h >= ax.nh || t0 < 0 || t0 >= ax.nt) return;
  for (int k = 0; k <= snap; k++) {
    const long long t = t0 - (long long)ax.sign * k;
    if (t < 0 || t >= ax.nt) return;  // the walk never leaves the region
    const long long row = h * ax.bh + t * ax.bt;
    if ((G[row * ax.wpr + (x >> 6)] >> (x & 63)) & 1ull) {
      store_cost(cost + h * ax.sh + t * ax.st + x, 0);
      atomicAdd(&ctl->seeds_used, 1);
      const int tx = (int)(x / kTileX), th = (int)(h / kTileH), tt = (int)(t / kTileT);
      const int lx = (int)(x % kTileX), lh = (int)(h % kTileH), lt = (int)(t % kTileT);
      const int tile = (tt * ax.tiles_h + th) * ax.tiles_x + tx;
      for (int level = -1; level <= 1; level++) {  // the tiles that hold the cell or see it in their halo
        if (level < 0 && !(lt < S && tt > 0)) continue;
        if (level > 0 && !(lt >= kTileT - S && tt + 1 < ax.tiles_t)) continue;
        const int at = tile + level * ax.tiles_x * ax.tiles_h;
        flags[at] = 1;
        if (lx == 0 && tx > 0) flags[at - 1] = 1;
        if (lx == kTileX - 1 && tx + 1 < ax.tiles_x) flags[at + 1] = 1;
        if (lh == 0 && th > 0) flags[at - ax.tiles_x] = 1;
        if (lh == kTileH - 1 && th + 1 < ax.tiles_h) flags[at + ax.tiles_x] = 1;
      }
      return;
    }
  }
}

// flags_now: this round's (a tile clears its own), flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void ground_relax_kernel(int32_t *__restrict__ cost, const u64 *__restrict__ G, GroundAxes ax, int S, int c,
                                                           int *__restrict__ flags_now, int *__restrict__ flags_next,
                                                           GroundControl *__restrict__ ctl) {
  extern __shared__ int32_t s[];  // (kTileT + 2 S) layers of kLayer values
  __shared__ u64 row_bits[kTileRows];  // row r = t * 8 + h
  __shared__ int go, faces;
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  if (tid == 0) {
    go = flags_now[tile];
    flags_now[tile] = 0;
    faces = 0;
  }
  __syncthreads();
  if (!go) return;
  const int tx = tile % ax.tiles_x, th = (tile / ax.tiles_x) % ax.tiles_h, tt = tile / (ax.tiles_x * ax.tiles_h);
  const int x0 = tx * kTileX, h0 = th * kTileH, t0 = tt * kTileT;
  const int gx = x0 + lane;

  // stage: staged row r = pt * 10 + ph is the row h0 + ph - 1, t0 + pt - S of the region; outside the region: "none"
  for (int r = w; r < (kTileT + 2 * S) * kRowsH; r += 4) {
    const int ph = r % kRowsH, pt = r / kRowsH;
    const int gh = h0 + ph - 1, gt = t0 + pt - S;
    const bool row_in = gh >= 0 && gh < ax.nh && gt >= 0 && gt < ax.nt;
    const int32_t *__restrict__ row = cost + gh * ax.sh + gt * ax.st;
    s[r * kRowPitch + 1 + lane] = row_in && gx < ax.nx ? load_cost(row + gx) : kNone;
    if (lane == 0) s[r * kRowPitch] = row_in && x0 > 0 ? load_cost(row + x0 - 1) : kNone;
    if (lane == 63) s[r * kRowPitch + kTileX + 1] = row_in && x0 + kTileX < ax.nx ? load_cost(row + x0 + kTileX) : kNone;
  }
  if (tid < kTileRows) {
    const int gh = h0 + (tid & 7), gt = t0 + (tid >> 3);
    row_bits[tid] = gh < ax.nh && gt < ax.nt ? G[((long long)gh * ax.bh + (long long)gt * ax.bt) * ax.wpr + tx] : 0ull;
  }
  __syncthreads();

  int again;
  do {
    int changed = 0;
    for (int colour = 0; colour < 2; colour++) {
      // a wavefront per pair of rows h = 2 p, 2 p + 1 of one t: the lane's cell has (x + h) & 1 == colour
      for (int p = w; p < kTileRows / 2; p += 4) {
        const int t = p >> 2, h = ((p & 3) << 1) | ((lane ^ colour) & 1);
        if ((row_bits[t * 8 + h] >> lane) & 1ull) {
          const int at = ((t + S) * kRowsH + h + 1) * kRowPitch + 1 + lane;
          const int before = s[at];
          int v = before;
          for (int j = -S; j <= S; j++) {
            const int o = at + j * kLayer;
            const int low = min(min(s[o - 1], s[o + 1]), min(s[o - kRowPitch], s[o + kRowPitch]));
            v = min(v, low + 1 + c * (j < 0 ? -j : j));
          }
          if (v < before) { s[at] = v; changed = 1; }
        }
      }
      __syncthreads();
    }
    again = __syncthreads_or(changed);
  } while (again);

  // write back what fell; which neighbours see it: bit 3 * side + level, side -x +x -h +h, level below, same, above; bits 12 and 13:
  // the tile straight below and above; bit 14: anything fell
  int mine = 0;
  for (int r = w; r < kTileRows; r += 4) {
    const int h = r & 7, t = r >> 3;
    if (!((row_bits[r] >> lane) & 1ull)) continue;  // a set bit: the cell is inside the region
    const int v = s[((t + S) * kRowsH + h + 1) * kRowPitch + 1 + lane];
    int32_t *p = cost + (h0 + h) * ax.sh + (t0 + t) * ax.st + gx;
    if (v < load_cost(p)) {
      store_cost(p, v);
      mine |= 1 << 14;
      int levels = 2;
      if (t < S && tt > 0) levels |= 1;
      if (t >= kTileT - S && tt + 1 < ax.tiles_t) levels |= 4;
      mine |= (levels & 1) << 12 | (levels & 4) << 11;
      if (lane == 0 && tx > 0) mine |= levels;
      if (lane == 63 && tx + 1 < ax.tiles_x) mine |= levels << 3;
      if (h == 0 && th > 0) mine |= levels << 6;
      if (h == kTileH - 1 && th + 1 < ax.tiles_h) mine |= levels << 9;
    }
  }
  if (mine) atomicOr(&faces, mine);
  __syncthreads();
  const int f = faces;
  if (tid < 14 && ((f >> tid) & 1)) {
    const int side = tid / 3, level = tid < 12 ? tid % 3 - 1 : tid == 12 ? -1 : 1;
    const int step = side == 0 ? -1 : side == 1 ? 1 : side == 2 ? -ax.tiles_x : side == 3 ? ax.tiles_x : 0;
    flags_next[tile + step + level * ax.tiles_x * ax.tiles_h] = 1;
  }
  if (tid == 0) {
    if (f) atomicAdd(&ctl->changed_tiles, 1ull);
    atomicAdd(&ctl->tile_runs, 1ull);
  }
}

__global__ __launch_bounds__(256) void ground_finish_kernel(int32_t *__restrict__ cost, int nx, int wpr, long long words,
                                                            const u64 *__restrict__ G) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  if (x >= nx) return;
  const long long at = (word / wpr) * nx + x;
  const int v = cost[at];
  cost[at] = !((G[word] >> lane) & 1ull) ? -2 : v == kNone ? -1 : v;
}

// one lane per start.  Every index read lies inside the region: a cell is looked at only after its coordinates were tested.
__global__ __launch_bounds__(256) void trace_ground_paths_kernel(const int32_t *__restrict__ field, long long ox, long long oy, long long oz,
                                                                 long long nx, long long nh, long long nt, long long sh, long long st,
                                                                 int up_axis, int sign, int S, int c, int snap,
                                                                 const int32_t *__restrict__ starts, int n, int max_cells,
                                                                 int32_t *__restrict__ paths, int32_t *__restrict__ lengths) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  long long x = (long long)starts[3 * i] - ox;
  const long long sy = (long long)starts[3 * i + 1] - oy, sz = (long long)starts[3 * i + 2] - oz;
  long long h = up_axis == 1 ? sz : sy, t = up_axis == 1 ? sy : sz;
  int len = 0, v = -2;
  if (x >= 0 && x < nx && h >= 0 && h < nh && t >= 0 && t < nt) {
    for (int k = 0; k <= snap && t >= 0 && t < nt; k++, t -= sign) {  // the first value other than -2, against u, inside the region
      v = field[h * sh + t * st + x];
      if (v != -2) break;
    }
  }
  if (v >= 0) {
    int32_t *out = paths + (long long)i * max_cells * 3;
    for (;;) {  // v falls strictly with every move and stays >= 0
      if (len < max_cells) {
        out[3 * len] = (int32_t)(x + ox);
        out[3 * len + 1] = (int32_t)((up_axis == 1 ? t : h) + oy);
        out[3 * len + 2] = (int32_t)((up_axis == 1 ? h : t) + oz);
      }
      len++;
      if (v == 0) break;
      bool moved = false;
      for (int e = 0; e < 4 && !moved; e++) {
        const long long x2 = x + (e == 0 ? -1 : e == 1 ? 1 : 0), h2 = h + (e == 2 ? -1 : e == 3 ? 1 : 0);
        if (x2 < 0 || x2 >= nx || h2 < 0 || h2 >= nh) continue;
        for (int m = 0; m <= 2 * S; m++) {  // j = 0, -1, +1, -2, +2, ...
          const int a = (m + 1) >> 1, j = (m & 1) ? -a : a;
          const long long t2 = t + (long long)sign * j;
          if (t2 < 0 || t2 >= nt) continue;
          const int v2 = field[h2 * sh + t2 * st + x2];
          if (v2 >= 0 && (long long)v2 + 1 + (long long)c * a == (long long)v) {
            x = x2, h = h2, t = t2, v = v2;
            moved = true;
            break;
          }
        }
      }
      if (!moved) { len = -len; break; }  // not a ground field: a cell above 0 without a predecessor
    }
  }
  lengths[i] = len;
}

struct SlotsRollback {  // what this call grew of the six slots does not stay behind a failure
  DeviceBuffer *slots[6];
  size_t had[6];
  explicit SlotsRollback(svoslam_workspace *ws)
      : slots{&ws->ground_bits, &ws->ground_a, &ws->ground_b, &ws->ground_body, &ws->ground_foot, &ws->ground_ctl} {
    for (int k = 0; k < 6; k++) had[k] = slots[k]->bytes;
  }
  int undo(int rc, hipStream_t stream) {  // the call's launches have finished before their slots go
    (void)hipStreamSynchronize(stream);
    for (int k = 0; k < 6; k++)
      if (slots[k]->bytes != had[k]) slots[k]->release();
    return rc;
  }
};

bool ground_parameters_valid(int up, int S, int c, int snap) {
  return up >= 2 && up <= 5 && S >= 0 && S <= SVOSLAM_MAX_STEP_CELLS && c >= 0 && c <= SVOSLAM_MAX_RING_COST && snap >= 0 &&
         snap <= SVOSLAM_MAX_SNAP_CELLS;
}

}  // namespace

int pool_ground_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                      int32_t up, int32_t r, int32_t H, int32_t S, int32_t c, int32_t snap, const int32_t *d_seeds, int32_t n_seeds,
                      int32_t *d_cost, svoslam_ground_stats *stats, hipStream_t stream) {
  if (stats) stats->footholds = stats->seeds_used = stats->rounds = stats->tile_runs = 0;
  if (!ws || !ground_parameters_valid(up, S, c, snap) || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || H < 1 || H > SVOSLAM_MAX_HEIGHT_CELLS ||
      S > H - 1 || n_seeds < 0 || (n_seeds > 0 && !d_seeds))
    return SVOSLAM_ERR_INVALID_ARG;
  const int ua = up >> 1, ha = 3 - ua, sign = (up & 1) ? -1 : 1;
  int below[3] = {r, r, r}, above[3] = {r, r, r};
  below[ua] = sign > 0 ? 1 : H - 1;
  above[ua] = sign > 0 ? H - 1 : 1;
  RegionPlan p;  // the region inflated by r horizontally, 1 below and H - 1 above
  SVO_TRY(plan_region_axes(depth, origin, dims, below, above, ha, &p));
  if (p.nothing) return SVOSLAM_OK;
  if (!d_cost) return SVOSLAM_ERR_INVALID_ARG;
  const long long nx = p.nx, ny = p.ny, nz = p.nz;
  const long long wpr = (nx + 63) / 64, words = wpr * ny * nz;  // the bit rows of the region itself
  const long long body_rows = r > 0 ? p.n_g2 / nx : 0, body_words = body_rows * wpr;
  GroundAxes ax;
  ax.nx = (int)nx, ax.ny = (int)ny, ax.up_axis = ua, ax.sign = sign, ax.wpr = (int)wpr;
  ax.nh = (int)(ua == 1 ? nz : ny), ax.nt = (int)(ua == 1 ? ny : nz);
  ax.sh = ua == 1 ? ny * nx : nx, ax.st = ua == 1 ? nx : ny * nx;
  ax.bh = ua == 1 ? (int)ny : 1, ax.bt = ua == 1 ? 1 : (int)ny;
  const long long tiles_x = wpr, tiles_h = (ax.nh + kTileH - 1) / kTileH, tiles_t = (ax.nt + kTileT - 1) / kTileT;
  const long long tiles = tiles_x * tiles_h * tiles_t;
  ax.tiles_x = (int)tiles_x, ax.tiles_h = (int)tiles_h, ax.tiles_t = (int)tiles_t;
  // the pool, the 2^31 - 1 limits of the cells and the raster's row words, then the drain of pending fusions
  SVO_TRY(admit_region("svoslam_pool_ground_field", pool, p, r, false, stream));
  // decided here, before anything is allocated or written
  if (r > 0 && !planar_within_limits(p, ha)) {
    set_last_error_text("svoslam_pool_ground_field: the region inflated by %d cells horizontally and %d along up (%lld x %lld x %lld) needs "
                        "an intermediate of more than 2^31 - 1 elements", r, H, p.len[0], p.len[1], p.len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (tiles * 256 > 0xFFFFFFFFll) {
    set_last_error_text("svoslam_pool_ground_field: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)", nx, ny,
                        nz, tiles);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (p.n_out * (1 + (long long)c * S) >= (long long)kNone) {
    set_last_error_text("svoslam_pool_ground_field: %lld cells at up to %lld a move could cost 2^30 or more, the value of \"not reached\"",
                        p.n_out, 1 + (long long)c * S);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  SlotsRollback grown(ws);
  const size_t flag_bytes = (size_t)tiles * 8;
  int rc = ws->ground_bits.reserve((size_t)p.words * 8);
  if (rc == SVOSLAM_OK && r > 0) rc = ws->ground_a.reserve((size_t)p.n_g1 * 4);
  if (rc == SVOSLAM_OK && r > 0) rc = ws->ground_b.reserve((size_t)p.n_g2 * 4);
  if (rc == SVOSLAM_OK && r > 0) rc = ws->ground_body.reserve((size_t)body_words * 8);
  if (rc == SVOSLAM_OK) rc = ws->ground_foot.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->ground_ctl.reserve(kControlBytes + flag_bytes);
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  u64 *O = ws->ground_bits.as<u64>(), *G = ws->ground_foot.as<u64>();
  const u64 *D = O;  // r = 0: the raster itself
  GroundControl *ctl = ws->ground_ctl.as<GroundControl>();
  int *flags = reinterpret_cast<int *>(ws->ground_ctl.as<char>() + kControlBytes);
  StageScope query(kStageQuery, stream);
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes + flag_bytes, stream));
  SVO_TRY(region_raster(pool, depth, p, false, O, stream));
  BodyRows b;
  b.off_x = p.off[0], b.off_h = p.off[ha], b.off_t = p.off[ua], b.len_t = (int)p.len[ua], b.wpr_o = (int)p.wpr;
  b.oh = ua == 1 ? (int)p.len[1] : 1, b.ot = ua == 1 ? 1 : (int)p.len[1];
  b.dh = b.oh, b.dt = b.ot;
  if (r > 0) {
    int32_t *within = ws->ground_b.as<int32_t>();  // per layer of t: the squared horizontal distance, -1 beyond r
    SVO_TRY(region_transform_planar(p, r, ha, O, ws->ground_a.as<int32_t>(), within, stream));
    RegionPlan rows = {};  // the transform's output as rows of nx values
    rows.nx = nx, rows.wpr = wpr, rows.words = body_words;
    SVO_TRY(region_pack(rows, within, true, nullptr, ws->ground_body.as<u64>(), stream));
    D = ws->ground_body.as<u64>();
    b.dh = ua == 1 ? (int)p.len[1] : 1, b.dt = ua == 1 ? 1 : (int)ny;  // [nz][len y][nx] or [len z][ny][nx]
  }
  ground_mask_kernel<<<cdiv(words, 256), 256, 0, stream>>>(O, D, ax, b, H, S, words, G, d_cost, ctl);
  SVO_LAUNCH_CHECK();
  if (n_seeds > 0) {
    ground_seed_kernel<<<cdiv(n_seeds, 256), 256, 0, stream>>>(d_seeds, n_seeds, origin[0], origin[1], origin[2], ax, S, snap, G, d_cost,
                                                               flags, ctl);
    SVO_LAUNCH_CHECK();
  }
  // rounds: a round in which no tile lowered anything is the last.  After round k every foothold with a cheapest chain that leaves a
  // tile at most k times is final, and a chain has fewer cells than the region, so the cap below is never reached; it keeps the
  // loop from spinning whatever happens.
  const long long cap = tiles * (long long)(kTileX * kTileH * kTileT) + 1;
  const size_t lds = (size_t)(kTileT + 2 * S) * kLayer * 4;
  GroundControl seen = {};
  u64 changed_before = 0;
  long long rounds = 0;
  for (;;) {
    if (rounds >= cap) {
      set_last_error_text("svoslam_pool_ground_field: no convergence after %lld rounds over %lld tiles", rounds, tiles);
      return SVOSLAM_ERR_HIP;
    }
    int *now = flags + (rounds & 1) * tiles, *next = flags + ((rounds + 1) & 1) * tiles;
    ground_relax_kernel<<<(unsigned)tiles, 256, lds, stream>>>(d_cost, G, ax, S, c, now, next, ctl);
    SVO_LAUNCH_CHECK();
    rounds++;
    SVO_HIP(hipMemcpyAsync(&seen, ctl, sizeof(seen), hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    if (seen.changed_tiles == changed_before) break;
    changed_before = seen.changed_tiles;
  }
  ground_finish_kernel<<<cdiv(words, 4), 256, 0, stream>>>(d_cost, (int)nx, (int)wpr, words, G);
  SVO_LAUNCH_CHECK();
  if (stats) {
    stats->rounds = (int32_t)(rounds < INT_MAX ? rounds : INT_MAX);
    stats->tile_runs = (int32_t)(seen.tile_runs < (u64)INT_MAX ? seen.tile_runs : (u64)INT_MAX);
    stats->seeds_used = seen.seeds_used;
    stats->footholds = seen.footholds;
  }
  return SVOSLAM_OK;
}

int field_trace_ground_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], int32_t up, int32_t S, int32_t c,
                             int32_t snap, const int32_t *d_starts, int32_t n_starts, int32_t max_cells, int32_t *d_paths,
                             int32_t *d_lengths, hipStream_t stream) {
  if (!origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n_starts < 0 || max_cells < 0 || !ground_parameters_valid(up, S, c, snap))
    return SVOSLAM_ERR_INVALID_ARG;
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  const long long plane = empty ? 0 : (long long)dims[0] * dims[1];  // below 2^62; the third factor only after it was tested
  const long long cells = plane > INT_MAX ? plane : plane * dims[2];
  if (cells > INT_MAX) {
    set_last_error_text("svoslam_field_trace_ground_paths: %d x %d x %d cells are more than 2^31 - 1", dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if ((long long)n_starts * max_cells > INT_MAX / 3) {
    set_last_error_text("svoslam_field_trace_ground_paths: %d starts of %d cells are more than 2^31 - 1 path entries", n_starts, max_cells);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_starts == 0) return SVOSLAM_OK;
  if (!d_starts || !d_lengths || (cells > 0 && !d_field) || (max_cells > 0 && !d_paths)) return SVOSLAM_ERR_INVALID_ARG;
  const int ua = up >> 1;
  const long long nx = dims[0], ny = dims[1], nz = dims[2];
  StageScope timed(kStageQuery, stream);
  trace_ground_paths_kernel<<<cdiv(n_starts, 256), 256, 0, stream>>>(
      d_field, origin[0], origin[1], origin[2], nx, ua == 1 ? nz : ny, ua == 1 ? ny : nz, ua == 1 ? ny * nx : nx, ua == 1 ? nx : ny * nx, ua,
      (up & 1) ? -1 : 1, S, c, snap, d_starts, n_starts, max_cells, d_paths, d_lengths);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
