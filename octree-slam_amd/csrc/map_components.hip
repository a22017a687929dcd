// map_components.hip -- the component labels of a map region: for every cell of a box of cells that is in the set S (the
// traversable cells T of the reach field, or the region's other cells) the smallest output index of any cell of its 6-connected
// component inside the region, -1 elsewhere; optionally the component's size at every cell (own specification, DESIGN.md section
// 17: the reference has nothing like it; the restatement the device must equal value for value is tests/test_components_cpu.py).
// A cell is in T iff svoslam_pool_distance_field with R = clearance_cells writes -1 there, so the field is computed first, by the
// existing host function and its kernels, into d_labels itself; everything after it is integers on the region: a union-find whose
// parent array is d_labels.
//
//   the pack                   map_region.hip's region_pack_kernel<false>: (dist2 == -1) != solid as the row words of S, for the
//                              region itself.
//   components_tile_kernel     one workgroup of 256 per tile of 64 x 8 x 8 cells.  The 64 row words and one int32 per cell live in
//                              LDS (16 KB + 512 B, no halo; a row is 64 consecutive dwords, so every access is conflict-free).  A
//                              cell of S starts with its own output index, every other cell with "none".  One pass = three sweeps
//                              with a barrier between them (map_sweeps.hpp, with a step of 0): x, a wavefront per row, sweep_row's
//                              minimum over the run of set bits; y and z, a lane per column, sweep_column's serial minimum up and
//                              down the 8 cells.  Passes repeat until one lowers nothing (a workgroup-wide OR): every
//                              pass lowers a value or is the last.  Each cell of S then stores its tile-local minimum: that is the
//                              parent array, parent[q] <= q, and a tile-local root points at itself.  Other cells store -1.
//   components_merge_kernel    one lane per cell on the low side of a tile face (x = 63 mod 64, y = 7 mod 8, z = 7 mod 8) that has a
//                              cell beyond it in the region.  If both cells are in S (read from the row words) the lane unites their
//                              trees without a lock: find follows parent with relaxed agent-scope atomic loads until parent[x] == x
//                              (the indices fall strictly); union puts the larger root under the smaller with atomicMin(&parent[hi],
//                              lo) and, if the old value was not hi -- somebody lowered it meanwhile --, goes on with the old value
//                              and lo, which are both smaller than hi.  On a y or z face a pair whose predecessor in x (same row
//                              word) is a pair too is skipped: the two rows' runs are joined by the predecessor.
//   components_flatten_kernel  one lane per cell: labels[q] = find(q) in place, relaxed atomic loads and stores; a chain entry is
//                              only ever replaced by one of its ancestors.  Roots are counted with one atomicAdd per wavefront
//                              (ballot + popcount) into the 32-byte control record.
//   components_count_kernel    (only with d_sizes, zeroed before) a wavefront walks 16 chunks of 64 consecutive cells; the head lane
//                              of each run of equal labels in a chunk does one atomicAdd(&sizes[label], run length), and chunks of
//                              one label that follow each other are carried along and added once: a large component's root is
//                              one address, and this keeps the adds to it at one per 1024 cells.
//   components_spread_kernel   sizes[q] = sizes[labels[q]], or 0, over the same strips: only root entries are read by others, and
//                              a root rewrites its own value unchanged; the largest size is one atomicMax per wavefront that
//                              holds a root.
//
// Why the result is the canonical labelling.  parent[q] <= q holds always: a cell starts at its own index, the tile kernel stores
// a minimum that includes it, and atomicMin only lowers.  A link only ever puts a root under a smaller index of the same
// component (both ends of a united pair are face neighbours in S and in the region, or roots of their trees), so a tree never
// leaves its component and each tree's root is its minimum.  When atomicMin replaces parent[hi] = old by lo, the edge hi - old
// is dropped, hi - lo is made, and the lane goes on to unite old and lo: what was joined stays joined once the lane is done.
// After the merge launch every face-adjacent pair of S lies in one tree: inside a tile by the tile kernel's fixed point, across a
// face by the pair's own lane, or, for a skipped pair, through its predecessor pair and the two x contacts, which the tile kernel
// or an x-face lane (never skipped) has joined.  So the trees are exactly the components, whatever the order of workgroups, and
// the label is the component's smallest output index.
//
// No cooperative launch, no workgroup waits on memory another writes, no persistent kernel, no inline assembly, no per-lane
// arrays indexed at run time.  Every device loop ends by its own data: a find's indices fall strictly, a union continues only
// with smaller indices, a tile pass lowers a value or is the last.  The call is asynchronous unless stats are asked for.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950), scratch 0 bytes for every kernel:
//   components_tile_kernel     58 VGPRs, 69 SGPRs, 17152 bytes of static LDS (9 workgroups per CU of 160 KB), occupancy 8
//   components_merge_kernel    15 VGPRs, 40 SGPRs, no LDS, occupancy 8
//   components_flatten_kernel  10 VGPRs, 18 SGPRs, no LDS, occupancy 8
//   components_count_kernel    16 VGPRs, 30 SGPRs, no LDS, occupancy 8
//   components_spread_kernel   14 VGPRs, 20 SGPRs, no LDS, occupancy 8
#include <limits.h>

#include "map_components.hpp"
#include "map_field.hpp"
#include "map_region.hpp"
#include "map_sweeps.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr int kNone = INT_MAX;                 // not in S (LDS only; an output index is <= 2^31 - 2)
constexpr int kTileX = 64, kTileY = 8, kTileZ = 8;
constexpr int kRows = kTileY * kTileZ;
constexpr int kStrip = 16;                     // chunks of 64 cells a wavefront of the two size kernels walks

struct ComponentControl {  // read back once, and only when the caller asks for stats
  unsigned long long tile_passes;
  int32_t components, largest, unions, pad;
};
constexpr size_t kControlBytes = 32;
static_assert(sizeof(ComponentControl) <= kControlBytes, "the control record has a slot of 32 bytes");

__device__ inline int load_parent(const int32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ inline void store_parent(int32_t *p, int v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ inline int find_root(const int32_t *parent, int x) {  // the indices fall strictly until parent[x] == x
  for (;;) {
    const int p = load_parent(parent + x);
    if (p == x) return x;
    x = p;
  }
}

__global__ __launch_bounds__(256) void components_tile_kernel(int32_t *__restrict__ labels, const unsigned long long *__restrict__ bits, int nx,
                                                              int ny, int nz, int wpr, int tiles_x, int tiles_y,
                                                              ComponentControl *__restrict__ ctl) {
  __shared__ int32_t s[kRows * kTileX];
  __shared__ unsigned long long row_bits[kRows];
  const int tile = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int tx = tile % tiles_x, ty = (tile / tiles_x) % tiles_y, tz = tile / (tiles_x * tiles_y);
  const int x0 = tx * kTileX, y0 = ty * kTileY, z0 = tz * kTileZ;
  const int gx = x0 + lane;
  unsigned long long mine = 0ull;
  if (tid < kRows) {
    const int gy = y0 + (tid & 7), gz = z0 + (tid >> 3);
    mine = gy < ny && gz < nz ? bits[((long long)gz * ny + gy) * wpr + tx] : 0ull;
    row_bits[tid] = mine;
  }
  const int any = __syncthreads_or(mine != 0ull);  // also the barrier behind the row words
  // row r of the tile is y = r & 7, z = r >> 3, at dwords r * 64 .. r * 64 + 63
  for (int r = w; r < kRows; r += 4)
    s[r * kTileX + lane] = (row_bits[r] >> lane) & 1ull ? (int)(((long long)(z0 + (r >> 3)) * ny + (y0 + (r & 7))) * nx + gx) : kNone;
  __syncthreads();

  int passes = 0, again = 0;
  if (any) do {
    int changed = 0;
    // x: a wavefront per row, the minimum over each run of set bits
    for (int r = w; r < kRows; r += 4) {
      const unsigned long long tw = row_bits[r];
      if (tw == 0ull) continue;  // the same for the whole wavefront
      const int at = r * kTileX + lane;
      const int before = s[at];
      const int v = sweep_row<0>(before, tw, lane);
      if (v < before) { s[at] = v; changed = 1; }
    }
    __syncthreads();
    // y: a lane per (x, z) column
    for (int z = w; z < kTileZ; z += 4) {
      int32_t *col = s + z * kTileY * kTileX + lane;
      changed |= sweep_column<0, kNone, kTileX, 1, true>(col, row_bits + z * 8, lane, kNone);
      changed |= sweep_column<0, kNone, kTileX, 1, false>(col, row_bits + z * 8, lane, kNone);
    }
    __syncthreads();
    // z: a lane per (x, y) column
    for (int y = w; y < kTileY; y += 4) {
      int32_t *col = s + y * kTileX + lane;
      changed |= sweep_column<0, kNone, kTileY * kTileX, 8, true>(col, row_bits + y, lane, kNone);
      changed |= sweep_column<0, kNone, kTileY * kTileX, 8, false>(col, row_bits + y, lane, kNone);
    }
    passes++;
    again = __syncthreads_or(changed);  // also the barrier in front of the next pass's x sweep
  } while (again);

  // the parent array: a cell of S its tile-local minimum, every other cell of the region -1
  if (gx < nx) {
    for (int r = w; r < kRows; r += 4) {
      const int gy = y0 + (r & 7), gz = z0 + (r >> 3);
      if (gy >= ny || gz >= nz) continue;
      const int v = s[r * kTileX + lane];
      labels[((long long)gz * ny + gy) * nx + gx] = v == kNone ? -1 : v;
    }
  }
  if (tid == 0 && passes) atomicAdd(&ctl->tile_passes, (unsigned long long)passes);
}

// faces_x, faces_y: the pairs across x faces, across y faces; the pairs across z faces follow up to `faces`
__global__ __launch_bounds__(256) void components_merge_kernel(int32_t *__restrict__ parent, const unsigned long long *__restrict__ bits, int nx,
                                                               int ny, int nz, int wpr, long long faces_x, long long faces_y, long long faces,
                                                               ComponentControl *__restrict__ ctl) {
  long long i = (long long)blockIdx.x * 256 + threadIdx.x;
  if (i >= faces) return;
  long long a, b;  // the pair's output indices, a < b
  if (i < faces_x) {  // (face, row): x = 64 * face + 63 and the cell after it, never skipped
    const long long row = i % ((long long)ny * nz);
    const int word = (int)(i / ((long long)ny * nz));
    const unsigned long long lo = bits[row * wpr + word], hi = bits[row * wpr + word + 1];
    if (!((lo >> 63) & hi & 1ull)) return;
    a = row * nx + word * 64 + 63;
    b = a + 1;
  } else {
    long long row_a, row_b;
    int x;
    if (i < faces_x + faces_y) {  // (face, z, x): y = 8 * face + 7 and the row after it
      i -= faces_x;
      x = (int)(i % nx);
      const long long zf = i / nx;
      row_a = (zf % nz) * ny + (zf / nz) * kTileY + kTileY - 1;
      row_b = row_a + 1;
    } else {  // (face, y, x): z = 8 * face + 7 and the plane after it
      i -= faces_x + faces_y;
      x = (int)(i % nx);
      const long long yf = i / nx;
      row_a = ((yf / ny) * kTileZ + kTileZ - 1) * ny + yf % ny;
      row_b = row_a + ny;
    }
    const unsigned long long both = bits[row_a * wpr + (x >> 6)] & bits[row_b * wpr + (x >> 6)];
    const int bit = x & 63;
    if (!((both >> bit) & 1ull)) return;
    if (bit > 0 && ((both >> (bit - 1)) & 1ull)) return;  // the predecessor pair joins the same two runs
    a = row_a * nx + x;
    b = row_b * nx + x;
  }
  int ra = (int)a, rb = (int)b;
  for (;;) {
    ra = find_root(parent, ra);
    rb = find_root(parent, rb);
    if (ra == rb) return;
    const int lo = min(ra, rb), hi = max(ra, rb);
    const int old = atomicMin(parent + hi, lo);
    if (old == hi) {  // hi was a root and is now under lo
      atomicAdd(&ctl->unions, 1);
      return;
    }
    ra = old;  // parent[hi] had fallen meanwhile and is now min(old, lo): old and lo, both below hi, are still to be joined
    rb = lo;
  }
}

__global__ __launch_bounds__(256) void components_flatten_kernel(int32_t *__restrict__ labels, long long n, ComponentControl *__restrict__ ctl) {
  const long long q = (long long)blockIdx.x * 256 + threadIdx.x;
  bool root = false;
  if (q < n) {
    const int p = load_parent(labels + q);
    if (p >= 0) {
      const int r = p == (int)q ? p : find_root(labels, p);
      if (r != p) store_parent(labels + q, r);
      root = r == (int)q;
    }
  }
  const unsigned long long roots = __ballot(root);
  if ((threadIdx.x & 63) == 0 && roots) atomicAdd(&ctl->components, __popcll(roots));
}

// a wavefront walks kStrip chunks of 64 consecutive cells.  A chunk of one label that continues the chunk before it is carried
// along and added once; every other chunk adds run by run
__global__ __launch_bounds__(256) void components_count_kernel(const int32_t *__restrict__ labels, long long n, int32_t *__restrict__ sizes) {
  const int lane = threadIdx.x & 63;
  const long long base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * kStrip);
  int carried = -1, carry = 0;  // the same in every lane
#pragma unroll 1
  for (int k = 0; k < kStrip; k++) {
    const long long q = base + k * 64 + lane;
    const int label = q < n ? labels[q] : -1;
    const int first = __builtin_amdgcn_readfirstlane(label);
    const bool uniform = __all(label == first);
    if (uniform && first == carried) {
      carry += 64;
      continue;
    }
    if (lane == 0 && carried >= 0) atomicAdd(sizes + carried, carry);
    carried = uniform ? first : -1;
    carry = uniform ? 64 : 0;
    if (uniform) continue;
    const int below = __shfl_up(label, 1);
    const bool head = lane == 0 || below != label;
    const unsigned long long heads = __ballot(head);
    if (head && label >= 0) {
      const unsigned long long rest = lane == 63 ? 0ull : heads >> (lane + 1);  // the heads above this lane
      atomicAdd(sizes + label, rest ? __ffsll((long long)rest) : 64 - lane);
    }
  }
  if (lane == 0 && carried >= 0) atomicAdd(sizes + carried, carry);
}

__global__ __launch_bounds__(256) void components_spread_kernel(const int32_t *__restrict__ labels, long long n, int32_t *sizes,
                                                                ComponentControl *__restrict__ ctl) {
  const int lane = threadIdx.x & 63;
  const long long base = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * (64 * kStrip);
  int at_root = 0;
#pragma unroll 1
  for (int k = 0; k < kStrip; k++) {
    const long long q = base + k * 64 + lane;
    if (q < n) {
      const int label = labels[q];
      const int size = label >= 0 ? sizes[label] : 0;
      sizes[q] = size;
      if (label == (int)q) at_root = max(at_root, size);
    }
  }
#pragma unroll
  for (int k = 32; k >= 1; k /= 2) at_root = max(at_root, __shfl_xor(at_root, k));
  if (lane == 0 && at_root > 0) atomicMax(&ctl->largest, at_root);
}

}  // namespace

int pool_label_components(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                          int32_t r, int32_t which, int32_t *d_labels, int32_t *d_sizes, svoslam_component_stats *stats,
                          hipStream_t stream) {
  if (stats) stats->components = stats->largest = stats->tile_passes = stats->unions = 0;
  if (!ws || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || (which != SVOSLAM_COMPONENTS_FREE && which != SVOSLAM_COMPONENTS_SOLID))
    return SVOSLAM_ERR_INVALID_ARG;
  RegionPlan own;  // the region itself: its row words are <= the field's own, within its limits
  SVO_TRY(plan_region(depth, origin, dims, 0, &own));
  if (own.nothing) return SVOSLAM_OK;
  if (!pool || !pool->d_data || !d_labels) return SVOSLAM_ERR_INVALID_ARG;  // argument errors come before the limits
  const long long nx = own.nx, ny = own.ny, nz = own.nz, n = own.n_out, wpr = own.wpr, words = own.words;
  const long long tiles_x = wpr, tiles_y = (ny + kTileY - 1) / kTileY, tiles_z = (nz + kTileZ - 1) / kTileZ;
  const long long tiles = tiles_x * tiles_y * tiles_z;
  // a launch takes at most 2^32 - 1 work-items: decided here, before anything is allocated or written
  if (n <= INT_MAX && tiles * 256 > 0xFFFFFFFFll) {
    set_last_error_text("svoslam_pool_label_components: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)",
                        nx, ny, nz, tiles);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  // the set, as the field's -1, in d_labels: the rest of the argument checks, the field's limits (decided before anything is
  // allocated), the drain of pending fusions and the field's own slots are pool_distance_field's
  SlotRollback grown(ws, &ws->comp_bits, &ws->comp_ctl);
  AdoptedBracket bracket(stream);
  SVO_TRY(pool_distance_field(ws, pool, depth, origin, dims, r, d_labels, nullptr, stream, &bracket.token));
  int rc = ws->comp_bits.reserve((size_t)words * 8);
  if (rc == SVOSLAM_OK) rc = ws->comp_ctl.reserve(kControlBytes);
  if (rc != SVOSLAM_OK) return grown.undo(rc, stream);
  unsigned long long *bits = ws->comp_bits.as<unsigned long long>();
  ComponentControl *ctl = ws->comp_ctl.as<ComponentControl>();
  SVO_HIP(hipMemsetAsync(ctl, 0, kControlBytes, stream));
  SVO_TRY(region_pack(own, d_labels, which == SVOSLAM_COMPONENTS_SOLID, nullptr, bits, stream));
  components_tile_kernel<<<(unsigned)tiles, 256, 0, stream>>>(d_labels, bits, (int)nx, (int)ny, (int)nz, (int)wpr, (int)tiles_x, (int)tiles_y,
                                                              ctl);
  SVO_LAUNCH_CHECK();
  const long long faces_x = (tiles_x - 1) * ny * nz, faces_y = (tiles_y - 1) * nx * nz, faces_z = (tiles_z - 1) * nx * ny;
  const long long faces = faces_x + faces_y + faces_z;  // < n / 64 + n / 8 + n / 8
  if (faces > 0) {
    components_merge_kernel<<<cdiv(faces, 256), 256, 0, stream>>>(d_labels, bits, (int)nx, (int)ny, (int)nz, (int)wpr, faces_x, faces_y, faces,
                                                                  ctl);
    SVO_LAUNCH_CHECK();
  }
  components_flatten_kernel<<<cdiv(n, 256), 256, 0, stream>>>(d_labels, n, ctl);
  SVO_LAUNCH_CHECK();
  if (d_sizes) {
    SVO_HIP(hipMemsetAsync(d_sizes, 0, (size_t)n * 4, stream));
    components_count_kernel<<<cdiv(n, 256 * kStrip), 256, 0, stream>>>(d_labels, n, d_sizes);
    SVO_LAUNCH_CHECK();
    components_spread_kernel<<<cdiv(n, 256 * kStrip), 256, 0, stream>>>(d_labels, n, d_sizes, ctl);
    SVO_LAUNCH_CHECK();
  }
  if (stats) {  // the one readback: with stats the call blocks
    ComponentControl seen = {};
    SVO_HIP(hipMemcpyAsync(&seen, ctl, sizeof(seen), hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    stats->components = seen.components;
    stats->largest = seen.largest;
    stats->tile_passes = (int32_t)(seen.tile_passes < (unsigned long long)INT_MAX ? seen.tile_passes : (unsigned long long)INT_MAX);
    stats->unions = seen.unions;
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
