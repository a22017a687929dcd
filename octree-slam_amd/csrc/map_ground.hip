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
//   ground_relax_kernel  map_relax.hpp's scheme over x, h, t with a halo of one cell along x and h and S cells along t: the staged
//                        costs are (8 + 2 S) * 10 * 66 values of dynamic LDS (21120 bytes at S = 0, 42240 at S = 4).  Its own: the
//                        pass and the flag rule.  A horizontal move flips the parity of x + h, so one pass is two
//                        half-passes by that parity with a barrier between: a lane writes only cells of the half-pass's colour and
//                        reads only the other colour (and halo cells, which nobody writes), free of races and deterministic.  Each
//                        wavefront takes the rows h = 2 p and 2 p + 1 of one t together, even lanes on one row and odd lanes on
//                        the other, so that all 64 lanes hold a cell of the colour; their LDS addresses fall on 64 different dwords
//                        with distinct banks per 32-lane half (pitch 66: an even lane x reads bank x, an odd lane x + 66 = x + 2 mod 32).
//                        A cell reads its 4 (2 S + 1) sources; a cell without its bit is skipped and holds "none", which no sum
//                        reaches from below.  Passes repeat until one changes nothing (__syncthreads_or).  The flags raised for
//                        a lowered cell: the horizontal face neighbour of a lowered border column; the
//                        tile above or below THAT one when the cell lies within S of the tile's top or bottom; and the tile
//                        straight above or below for any lowered cell within S of the top or bottom -- no move is vertical, but
//                        a move inside the tile's x and h range that climbs across its top lands there.  Up to 14 neighbours.
//   the rounds and the finish are map_relax.hpp's.
//
// field_trace_ground_paths: trace_ground_paths_kernel, one lane per start: the start is snapped like a seed (the first value other
// than -2), then from a cell of value v > 0 the walk takes the first candidate q + e + j u with a value v' >= 0 and v' + 1 + c |j|
// == v, e in the order -x +x -h +h and j = 0, -1, +1, -2, +2, ... within one e.  The values fall strictly.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): in DESIGN.md section 23.  Every kernel 0 bytes of scratch,
// no per-lane arrays indexed at run time, no inline assembly; every store is a vector store from plain C++.
#include "map_ground.hpp"
#include "map_region.hpp"
#include "map_relax.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

typedef unsigned long long u64;

struct GroundAxes {   // the region seen as x, h (the other horizontal axis) and t (the up axis)
  TileGrid g;         // with a = h and b = t
  int ny;             // decodes a bit row: row = z * ny + y
  int up_axis, sign;  // 1 = y, 2 = z; +1 or -1: u = sign * (unit vector of up_axis)
};

struct BodyRows {     // the rows of the inflated raster O and of the body bits D
  int off_x, off_h, off_t, len_t;  // the region's first cell inside the inflated one; inflated cells along t
  int wpr_o;                       // words per row of O
  int oh, ot, dh, dt;              // row strides of h' and t' in O, of h and t' in D
};

// 64 bits of a row of O from bit 64 * wi + shift on; behind the row's last word: zero
__device__ inline u64 shifted_word(const u64 *__restrict__ row, int wi, int shift, int wpr) {
  u64 v = row[wi] >> shift;
  if (shift && wi + 1 < wpr) v |= row[wi + 1] << (64 - shift);
  return v;
}

__global__ __launch_bounds__(256) void ground_mask_kernel(const u64 *__restrict__ O, const u64 *__restrict__ D, GroundAxes ax, BodyRows b,
                                                          int H, int S, long long words, u64 *__restrict__ G,
                                                          int32_t *__restrict__ cost, RelaxControl *__restrict__ ctl) {
  const int nx = ax.g.nx, wpr = ax.g.wpr;
  const long long word = (long long)blockIdx.x * 256 + threadIdx.x;
  if (word < words) {
    const int wx = (int)(word % wpr);
    const long long row = word / wpr;
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
        if (k >= S) g &= ~D[(hd + (long long)tk * b.dt) * wpr + wx];
      }
    }
    if (wx == wpr - 1 && (nx & 63)) g &= (1ull << (nx & 63)) - 1ull;  // bits behind the region's last x
    G[word] = g;
    if (g) atomicAdd(&ctl->footholds, __popcll(g));
  }
  // the cells of this workgroup's 256 words become "none": a wavefront per word, 64 consecutive values per store
  const int lane = threadIdx.x & 63;
  for (int i = threadIdx.x >> 6; i < 256; i += 4) {
    const long long wd = (long long)blockIdx.x * 256 + i;
    if (wd >= words) break;
    const int x = (int)(wd % wpr) * 64 + lane;
    if (x < nx) cost[(wd / wpr) * nx + x] = kNone;
  }
}

__global__ __launch_bounds__(256) void ground_seed_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, GroundAxes ax,
                                                          int S, int snap, const u64 *__restrict__ G, int32_t *__restrict__ cost,
                                                          int *__restrict__ flags, RelaxControl *__restrict__ ctl) {
  const TileGrid &g = ax.g;
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, y = (long long)seeds[3 * i + 1] - oy, z = (long long)seeds[3 * i + 2] - oz;
  const long long h = ax.up_axis == 1 ? z : y, t0 = ax.up_axis == 1 ? y : z;
  if (x < 0 || x >= g.nx || h < 0 || h >= g.na || t0 < 0 || t0 >= g.nb) return;
  for (int k = 0; k <= snap; k++) {
    const long long t = t0 - (long long)ax.sign * k;
    if (t < 0 || t >= g.nb) return;  // the walk never leaves the region
    const long long row = h * g.ba + t * g.bb;
    if ((G[row * g.wpr + (x >> 6)] >> (x & 63)) & 1ull) {
      store_value(cost + h * g.sa + t * g.sb + x, 0);
      atomicAdd(&ctl->seeds_used, 1);
      const int tx = (int)(x / kTileX), th = (int)(h / kTileA), tt = (int)(t / kTileB);
      const int lx = (int)(x % kTileX), lh = (int)(h % kTileA), lt = (int)(t % kTileB);
      const int tile = (tt * g.tiles_a + th) * g.tiles_x + tx;
      for (int level = -1; level <= 1; level++) {  // the tiles that hold the cell or see it in their halo
        if (level < 0 && !(lt < S && tt > 0)) continue;
        if (level > 0 && !(lt >= kTileB - S && tt + 1 < g.tiles_b)) continue;
        const int at = tile + level * g.tiles_x * g.tiles_a;
        flags[at] = 1;
        if (lx == 0 && tx > 0) flags[at - 1] = 1;
        if (lx == kTileX - 1 && tx + 1 < g.tiles_x) flags[at + 1] = 1;
        if (lh == 0 && th > 0) flags[at - g.tiles_x] = 1;
        if (lh == kTileA - 1 && th + 1 < g.tiles_a) flags[at + g.tiles_x] = 1;
      }
      return;
    }
  }
}

// flags_now: this round's, flags_next: the coming round's (all clear when the launch starts)
__global__ __launch_bounds__(256) void ground_relax_kernel(int32_t *__restrict__ cost, const u64 *__restrict__ G, TileGrid g, int S, int c,
                                                           int *__restrict__ flags_now, int *__restrict__ flags_next,
                                                           RelaxControl *__restrict__ ctl) {
  extern __shared__ int32_t s[];  // (kTileB + 2 S) layers of kLayer values
  __shared__ u64 row_bits[kTileRows];  // row r = t * 8 + h
  __shared__ TileShared sh;
  if (!relax_enter(sh, flags_now)) return;
  const TileAt at = tile_at(g);
  relax_stage(s, row_bits, cost, G, g, at, S);
  __syncthreads();

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  int again;
  do {
    int changed = 0;
    for (int colour = 0; colour < 2; colour++) {
      // a wavefront per pair of rows h = 2 p, 2 p + 1 of one t: the lane's cell has (x + h) & 1 == colour
      for (int p = w; p < kTileRows / 2; p += 4) {
        const int t = p >> 2, h = ((p & 3) << 1) | ((lane ^ colour) & 1);
        if ((row_bits[t * 8 + h] >> lane) & 1ull) {
          const int cell = staged_at(h, t, S) + lane;
          const int before = s[cell];
          int v = before;
          for (int j = -S; j <= S; j++) {
            const int o = cell + j * kLayer;
            const int low = min(min(s[o - 1], s[o + 1]), min(s[o - kRowPitch], s[o + kRowPitch]));
            v = min(v, low + 1 + c * (j < 0 ? -j : j));
          }
          if (v < before) { s[cell] = v; changed = 1; }
        }
      }
      __syncthreads();
    }
    again = __syncthreads_or(changed);
  } while (again);

  // which neighbours see a lowered cell: bit 3 * side + level, side -x +x -h +h, level below, same, above; bits 12 and 13: the tile
  // straight below and above; bit 14: anything fell
  const int f = relax_store(cost, s, row_bits, sh, g, at, S, 1 << 14, [&](int lane, int h, int t) {
    int levels = 2;
    if (t < S && at.tb > 0) levels |= 1;
    if (t >= kTileB - S && at.tb + 1 < g.tiles_b) levels |= 4;
    int seen = (levels & 1) << 12 | (levels & 4) << 11;
    if (lane == 0 && at.tx > 0) seen |= levels;
    if (lane == 63 && at.tx + 1 < g.tiles_x) seen |= levels << 3;
    if (h == 0 && at.ta > 0) seen |= levels << 6;
    if (h == kTileA - 1 && at.ta + 1 < g.tiles_a) seen |= levels << 9;
    return seen;
  });
  if (tid < 14 && ((f >> tid) & 1)) {
    const int side = tid / 3, level = tid < 12 ? tid % 3 - 1 : tid == 12 ? -1 : 1;
    const int step = side == 0 ? -1 : side == 1 ? 1 : side == 2 ? -g.tiles_x : side == 3 ? g.tiles_x : 0;
    flags_next[at.tile + step + level * g.tiles_x * g.tiles_a] = 1;
  }
  relax_count(f, ctl);
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
  const char *fn = "svoslam_pool_ground_field";
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
  ax.ny = (int)ny, ax.up_axis = ua, ax.sign = sign;
  ax.g = ua == 1 ? tile_grid(nx, nz, ny, ny * nx, nx, ny, 1, wpr) : tile_grid(nx, ny, nz, nx, ny * nx, 1, ny, wpr);
  const long long tiles = ax.g.tiles();
  // the pool, the 2^31 - 1 limits of the cells and the raster's row words, then the drain of pending fusions
  SVO_TRY(admit_region(fn, pool, p, r, false, stream));
  // decided here, before anything is allocated or written
  if (r > 0 && !planar_within_limits(p, ha)) {
    set_last_error_text("svoslam_pool_ground_field: the region inflated by %d cells horizontally and %d along up (%lld x %lld x %lld) needs "
                        "an intermediate of more than 2^31 - 1 elements", r, H, p.len[0], p.len[1], p.len[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  SVO_TRY(relax_tile_limit(fn, ax.g, ny, nz));
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
  RelaxControl *ctl = ws->ground_ctl.as<RelaxControl>();
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
  const size_t lds = (size_t)(kTileB + 2 * S) * kLayer * 4;
  long long rounds;
  RelaxControl seen;
  SVO_TRY(relax_rounds(fn, tiles, ctl, flags, stream, [&](int *now, int *next) {
    ground_relax_kernel<<<(unsigned)tiles, 256, lds, stream>>>(d_cost, G, ax.g, S, c, now, next, ctl);
  }, &rounds, &seen));
  SVO_TRY(relax_finish(d_cost, nx, wpr, words, G, stream));
  if (stats) {
    relax_stats(stats, rounds, seen);
    stats->footholds = seen.footholds;
  }
  return SVOSLAM_OK;
}

int field_trace_ground_paths(const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], int32_t up, int32_t S, int32_t c,
                             int32_t snap, const int32_t *d_starts, int32_t n_starts, int32_t max_cells, int32_t *d_paths,
                             int32_t *d_lengths, hipStream_t stream) {
  if (!ground_parameters_valid(up, S, c, snap)) return SVOSLAM_ERR_INVALID_ARG;
  bool launch;
  SVO_TRY(trace_arguments("svoslam_field_trace_ground_paths", d_field, origin, dims, d_starts, n_starts, max_cells, d_paths, d_lengths,
                          &launch));
  if (!launch) return SVOSLAM_OK;
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
