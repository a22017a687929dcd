// map_coverage.hip -- viewpoints that cover a map region: which of n candidate cells see the most of a set of target cells, and a
// greedy set cover over them (own specification; the restatement the device must equal bit for bit is
// tests/test_coverage_cpu.py).  The sight rule is the visibility field's (section 19), the walk supercover_walk.hpp's.  Pure
// integers; ties go to the lowest candidate index.
//
// With the region inflated by max(R, 1) and clipped to the root (every cell between a counting candidate within range and its
// target lies in it, and so does every face neighbour of a region cell that lies in the root):
//   the raster           map_region.hip's region_raster_kernel: the occupied cells as 64-bit row words.
//   target_flag_kernel   one lane per region cell: 1 iff the cell passes the mode (surface: its own bit and the six neighbour bits
//                        of the raster; a neighbour outside the root is no cell) and the caller's select byte.
//   the ranks            exclusive_scan_u32 over the flags, in place; the total is T, read back once (4 bytes) to size the matrix.
//   target_emit_kernel   one lane per region cell: a target writes its region index at its rank; d_round gets -2 / -1.
//   sight_matrix_kernel  the hot path.  Row c of the matrix is candidate c, W = ceil(T / 64) words.  One wavefront answers the 64
//                        consecutive targets of one word: the candidate is uniform (read through readfirstlane), each lane takes
//                        the range test, a wavefront with nothing in range stores 0 and is done with the word, the others walk from
//                        the candidate towards their target.  The ballot of "seen" is the word, stored by lane 0 with one vector store; lanes
//                        past T and candidates outside the root vote 0.  Consecutive targets are neighbours in the region, so the
//                        walks of a wavefront start in the same cell and end next to each other.  The grid is bounded (at most 65535
//                        workgroups of four wavefronts): a wavefront takes word g, then g + the wavefronts of the grid, ..., so a
//                        matrix of up to 2^29 words is one launch of at most 2^24 work-items.
//   row_gain_kernel      one wavefront per candidate, the grid bounded and strided in the same way: the sum of popcount(row &
//                        ~covered) over the row, lanes striding the words, a shuffle reduction, then lane 0 writes d_seen (round 0: nothing is covered) and takes one 64-bit atomicMax
//                        into the round's record with the key gain << 32 | (2^32 - 1 - c): the largest key is the largest gain and
//                        among equal gains the lowest index.  A gain of 0 is not recorded (the record starts at 0, which decodes to
//                        gain 0), and a round after one that ended leaves at once: gains never rise.
//   coverable_kernel     one lane per word: the OR over the rows, its popcount reduced per wavefront, one atomicAdd into the summary.
//   cover_kernel         one lane per word: decodes the round's record; below min_gain nothing is written (the entries past the end
//                        were written when the call began).  Otherwise the row is ORed into `covered`, the newly covered bits get
//                        the round through the target list, and thread 0 writes d_chosen, d_gain and the running summary.
// All k_max rounds are queued without a readback; two launches a round.  A fused round and lazy gains were not built (section 24).
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): DESIGN.md section 24; every kernel 0 bytes of scratch, no
// LDS.  No per-lane arrays; every store is a vector store from plain C++.
#include <limits.h>

#include "map_coverage.hpp"
#include "map_region.hpp"
#include "radix_sort.hpp"
#include "stage_timing.hpp"
#include "supercover_walk.hpp"

namespace svoslam {

namespace {

constexpr long long kMaxMatrixWords = 1ll << 29;  // 4 GiB
constexpr long long kMaxGrid = 65535;             // workgroups of the two launches that grow with n_cands: their wavefronts stride

// the bit of cell (x, y, z) of the inflated region (coordinates relative to its first cell)
__device__ __forceinline__ bool occupied(const unsigned long long *__restrict__ bits, int wpr, int leny, int x, int y, int z) {
  return (bits[((long long)z * leny + y) * wpr + (x >> 6)] >> (x & 63)) & 1ull;
}

// (offx, offy, offz): the region's first cell inside the inflated one; (ox, oy, oz): the same cell in the root
__global__ __launch_bounds__(256) void target_flag_kernel(const unsigned long long *__restrict__ bits, int wpr, int leny, int offx,
                                                          int offy, int offz, int ox, int oy, int oz, int nx, int ny, int n_side,
                                                          int mode, const uint8_t *__restrict__ select, int total,
                                                          uint32_t *__restrict__ flags) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;  // total <= 2^31 - 1: the sum can pass it, compared unsigned
  if (lane_idx >= (unsigned)total) return;
  const int idx = (int)lane_idx;
  const int x = idx % nx, y = (idx / nx) % ny, z = idx / nx / ny;
  bool target = !select || select[idx] != 0;
  if (target && mode != SVOSLAM_COVER_ALL) {
    const int ix = x + offx, iy = y + offy, iz = z + offz;
    const bool occ = occupied(bits, wpr, leny, ix, iy, iz);
    if (mode == SVOSLAM_COVER_FREE) {
      target = !occ;
    } else if (!occ) {
      target = false;
    } else {  // a neighbour in the root lies in the inflated region: it is inflated by at least 1
      const int ax = ox + x, ay = oy + y, az = oz + z;
      bool open = false;
      if (ax > 0) open = !occupied(bits, wpr, leny, ix - 1, iy, iz);
      if (!open && ax + 1 < n_side) open = !occupied(bits, wpr, leny, ix + 1, iy, iz);
      if (!open && ay > 0) open = !occupied(bits, wpr, leny, ix, iy - 1, iz);
      if (!open && ay + 1 < n_side) open = !occupied(bits, wpr, leny, ix, iy + 1, iz);
      if (!open && az > 0) open = !occupied(bits, wpr, leny, ix, iy, iz - 1);
      if (!open && az + 1 < n_side) open = !occupied(bits, wpr, leny, ix, iy, iz + 1);
      target = open;
    }
  }
  flags[idx] = target ? 1u : 0u;
}

// ranks: the flags after the exclusive scan; *n_targets their sum
__global__ __launch_bounds__(256) void target_emit_kernel(const uint32_t *__restrict__ ranks, const uint32_t *__restrict__ n_targets,
                                                          int total, int32_t *__restrict__ list, int32_t *__restrict__ round) {
  const unsigned lane_idx = blockIdx.x * 256u + threadIdx.x;
  if (lane_idx >= (unsigned)total) return;
  const int idx = (int)lane_idx;
  const uint32_t rank = ranks[idx], next = idx + 1 < total ? ranks[idx + 1] : *n_targets;
  const bool target = next != rank;
  if (target) list[rank] = idx;
  if (round) round[idx] = target ? -2 : -1;
}

// what a call leaves where no round wrote: d_chosen -1, d_gain 0, d_seen 0 (NULL: not written), summary (T, 0, 0, 0)
__global__ __launch_bounds__(256) void cover_init_kernel(int k_max, int32_t *__restrict__ chosen, int32_t *__restrict__ gain, int n_seen,
                                                         int32_t *__restrict__ seen, int n_targets, int32_t *__restrict__ summary) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < (unsigned)k_max) {
    chosen[i] = -1;
    gain[i] = 0;
  }
  if (seen && i < (unsigned)n_seen) seen[i] = 0;
  if (i == 0) {
    summary[0] = n_targets;
    summary[1] = summary[2] = summary[3] = 0;
  }
}

// (lox, loy, loz), leny, wpr: the inflated region's first cell, rows per plane and words per row; (ox, oy, oz), nx, ny: the region
__global__ __launch_bounds__(256) void sight_matrix_kernel(const unsigned long long *__restrict__ bits, int wpr, int leny, int lox,
                                                           int loy, int loz, int ox, int oy, int oz, int nx, int ny, int n_side, int R,
                                                           const int32_t *__restrict__ cands, const int32_t *__restrict__ list,
                                                           int n_targets, int W, long long words,
                                                           unsigned long long *__restrict__ matrix) {
  const int lane = threadIdx.x & 63;
  // one wavefront per matrix word, striding by the wavefronts of the grid
  for (long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); word < words; word += (long long)gridDim.x * 4) {
    const int c = __builtin_amdgcn_readfirstlane((int)(word / W));
    const int t = (int)(word % W) * 64 + lane;
    const int vx = cands[3ll * c], vy = cands[3ll * c + 1], vz = cands[3ll * c + 2];
    const bool counts = (unsigned)vx < (unsigned)n_side && (unsigned)vy < (unsigned)n_side && (unsigned)vz < (unsigned)n_side;
    bool seen = false;
    int dx = 0, dy = 0, dz = 0;
    if (counts && t < n_targets) {
      const int idx = list[t];
      dx = ox + idx % nx - vx, dy = oy + (idx / nx) % ny - vy, dz = oz + idx / nx / ny - vz;
      const int ax = abs(dx), ay = abs(dy), az = abs(dz);
      seen = ax <= R && ay <= R && az <= R && ax * ax + ay * ay + az * az <= R * R;  // each term is then at most 4096^2
    }
    unsigned long long row_word = __ballot(seen);
    if (row_word != 0ull) {  // something of this word is in range
      if (seen)
        seen = !supercover_walk<long long>(vx - lox, vy - loy, vz - loz, dx, dy, dz,
                                           [&](int x, int y, int z) { return occupied(bits, wpr, leny, x, y, z); });
      row_word = __ballot(seen);
    }
    if (lane == 0) matrix[word] = row_word;
  }
}

// covered NULL: nothing is; prev: the record of the round before (NULL in round 0); rec NULL: only d_seen is wanted
__global__ __launch_bounds__(256) void row_gain_kernel(const unsigned long long *__restrict__ matrix, int W, int n_cands,
                                                       const unsigned long long *__restrict__ covered,
                                                       const unsigned long long *__restrict__ prev, int min_gain,
                                                       unsigned long long *__restrict__ rec, int32_t *__restrict__ seen) {
  if (prev && (long long)(*prev >> 32) < min_gain) return;  // the cover has ended: gains never rise
  const int lane = threadIdx.x & 63;
  // one wavefront per candidate, striding by the wavefronts of the grid
  for (long long c = (long long)blockIdx.x * 4 + (threadIdx.x >> 6); c < n_cands; c += (long long)gridDim.x * 4) {
    const unsigned long long *__restrict__ row = matrix + c * W;
    int sum = 0;
    for (int w = lane; w < W; w += 64) sum += __popcll(row[w] & ~(covered ? covered[w] : 0ull));
#pragma unroll
    for (int k = 32; k >= 1; k /= 2) sum += __shfl_xor(sum, k);
    if (lane == 0) {
      if (seen) seen[c] = sum;
      if (rec && sum > 0) atomicMax(rec, ((unsigned long long)sum << 32) | (0xFFFFFFFFull - (unsigned long long)c));
    }
  }
}

__global__ __launch_bounds__(256) void coverable_kernel(const unsigned long long *__restrict__ matrix, int W, int n_cands,
                                                        int32_t *__restrict__ summary) {
  const int w = (int)(blockIdx.x * 256u + threadIdx.x);
  unsigned long long any = 0ull;
  if (w < W)
    for (long long c = 0; c < n_cands; c++) any |= matrix[c * W + w];
  int sum = __popcll(any);
#pragma unroll
  for (int k = 32; k >= 1; k /= 2) sum += __shfl_xor(sum, k);
  if ((threadIdx.x & 63) == 0 && sum > 0) atomicAdd(&summary[3], sum);
}

__global__ __launch_bounds__(256) void cover_kernel(const unsigned long long *__restrict__ matrix, int W,
                                                    unsigned long long *__restrict__ covered,
                                                    const unsigned long long *__restrict__ rec, int min_gain, int j,
                                                    const int32_t *__restrict__ list, int32_t *__restrict__ round,
                                                    int32_t *__restrict__ chosen, int32_t *__restrict__ gain,
                                                    int32_t *__restrict__ summary) {
  const unsigned long long key = *rec;
  const int g = (int)(key >> 32);
  if (g < min_gain) return;  // past the end: those entries are already written
  const long long c = (long long)(0xFFFFFFFFull - (key & 0xFFFFFFFFull));
  const int w = (int)(blockIdx.x * 256u + threadIdx.x);
  if (w == 0) {
    chosen[j] = (int)c;
    gain[j] = g;
    summary[1] = j + 1;
    summary[2] += g;
  }
  if (w >= W) return;
  const unsigned long long before = covered[w], sees = matrix[c * W + w];
  unsigned long long fresh = sees & ~before;
  if (!fresh) return;
  covered[w] = before | sees;
  if (!round) return;
  while (fresh) {
    const int b = __builtin_ctzll(fresh);
    round[list[w * 64 + b]] = j;
    fresh &= fresh - 1;
  }
}

int init_outputs(int k_max, int32_t *d_chosen, int32_t *d_gain, int n_seen, int32_t *d_seen, int n_targets, int32_t *d_summary,
                 hipStream_t stream) {
  long long lanes = k_max > 1 ? k_max : 1;
  if (d_seen && n_seen > lanes) lanes = n_seen;
  cover_init_kernel<<<cdiv(lanes, 256), 256, 0, stream>>>(k_max, d_chosen, d_gain, n_seen, d_seen, n_targets, d_summary);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int cover(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const RegionPlan &p, const int32_t origin[3], int R, int mode,
          const uint8_t *d_select, const int32_t *d_cands, int n_cands, int k_max, int min_gain, int32_t *d_seen, int32_t *d_chosen,
          int32_t *d_gain, int32_t *d_round, int32_t *d_summary, hipStream_t stream) {
  const int n = (int)p.n_out;
  SVO_TRY(ws->cov_bits.reserve((size_t)p.words * 8));
  SVO_TRY(ws->cov_targets.reserve(((size_t)n * 2 + 2) * 4));  // the flags / ranks, the list, T
  unsigned long long *bits = ws->cov_bits.as<unsigned long long>();
  uint32_t *ranks = ws->cov_targets.as<uint32_t>(), *d_total = ranks + 2 * (size_t)n;
  int32_t *list = ws->cov_targets.as<int32_t>() + n;
  SVO_TRY(region_raster(pool, depth, p, false, bits, stream));
  target_flag_kernel<<<cdiv(n, 256), 256, 0, stream>>>(bits, (int)p.wpr, (int)p.len[1], p.off[0], p.off[1], p.off[2], origin[0], origin[1],
                                                       origin[2], (int)p.nx, (int)p.ny, 1 << depth, mode, d_select, n, ranks);
  SVO_LAUNCH_CHECK();
  SVO_TRY(exclusive_scan_u32(ws, ranks, (unsigned)n, d_total, stream));
  uint32_t n_targets = 0;  // the one readback: it sizes the matrix
  SVO_HIP(hipMemcpyAsync(&n_targets, d_total, sizeof(n_targets), hipMemcpyDeviceToHost, stream));
  SVO_HIP(hipStreamSynchronize(stream));
  const int T = (int)n_targets, W = (T + 63) / 64;
  const long long words = (long long)n_cands * W;
  if (words > kMaxMatrixWords) {
    set_last_error_text("svoslam_pool_cover_views: %d candidates x %d targets are a matrix of %lld words, more than 2^29", n_cands, T,
                        words);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (words > 0) {
    SVO_TRY(ws->cov_matrix.reserve((size_t)words * 8));
    SVO_TRY(ws->cov_state.reserve(((size_t)W + (size_t)k_max) * 8));
  }
  target_emit_kernel<<<cdiv(n, 256), 256, 0, stream>>>(ranks, d_total, n, list, d_round);
  SVO_LAUNCH_CHECK();
  SVO_TRY(init_outputs(k_max, d_chosen, d_gain, n_cands, words > 0 ? nullptr : d_seen, T, d_summary, stream));
  if (words == 0) return SVOSLAM_OK;  // no targets or no candidates: nothing is seen and nothing chosen
  unsigned long long *matrix = ws->cov_matrix.as<unsigned long long>();
  unsigned long long *covered = ws->cov_state.as<unsigned long long>(), *rec = covered + W;
  SVO_HIP(hipMemsetAsync(covered, 0, ((size_t)W + (size_t)k_max) * 8, stream));
  const unsigned word_grid = cdiv(words, 4) < kMaxGrid ? cdiv(words, 4) : (unsigned)kMaxGrid;
  const unsigned cand_grid = cdiv(n_cands, 4) < kMaxGrid ? cdiv(n_cands, 4) : (unsigned)kMaxGrid;
  sight_matrix_kernel<<<word_grid, 256, 0, stream>>>(bits, (int)p.wpr, (int)p.len[1], (int)p.lo[0], (int)p.lo[1], (int)p.lo[2],
                                                          origin[0], origin[1], origin[2], (int)p.nx, (int)p.ny, 1 << depth, R, d_cands,
                                                          list, T, W, words, matrix);
  SVO_LAUNCH_CHECK();
  coverable_kernel<<<cdiv(W, 256), 256, 0, stream>>>(matrix, W, n_cands, d_summary);
  SVO_LAUNCH_CHECK();
  if (k_max == 0 && d_seen) {  // no round: the scores alone
    row_gain_kernel<<<cand_grid, 256, 0, stream>>>(matrix, W, n_cands, nullptr, nullptr, min_gain, nullptr, d_seen);
    SVO_LAUNCH_CHECK();
  }
  for (int j = 0; j < k_max; j++) {
    row_gain_kernel<<<cand_grid, 256, 0, stream>>>(matrix, W, n_cands, covered, j ? rec + j - 1 : nullptr, min_gain, rec + j,
                                                   j ? nullptr : d_seen);
    SVO_LAUNCH_CHECK();
    cover_kernel<<<cdiv(W, 256), 256, 0, stream>>>(matrix, W, covered, rec + j, min_gain, j, list, d_round, d_chosen, d_gain, d_summary);
    SVO_LAUNCH_CHECK();
  }
  return SVOSLAM_OK;
}

}  // namespace

int pool_cover_views(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t R, int32_t mode, const uint8_t *d_select, const int32_t *d_cands, int32_t n_cands, int32_t k_max,
                     int32_t min_gain, int32_t *d_seen, int32_t *d_chosen, int32_t *d_gain, int32_t *d_round, int32_t *d_summary,
                     hipStream_t stream) {
  if (!ws || n_cands < 0 || (n_cands > 0 && !d_cands) || !d_summary) return SVOSLAM_ERR_INVALID_ARG;
  if (mode < SVOSLAM_COVER_SURFACE || mode > SVOSLAM_COVER_ALL) return SVOSLAM_ERR_INVALID_ARG;
  if (k_max < 0 || k_max > SVOSLAM_MAX_COVER_VIEWS || min_gain < 1) return SVOSLAM_ERR_INVALID_ARG;
  if (k_max > 0 && (!d_chosen || !d_gain)) return SVOSLAM_ERR_INVALID_ARG;
  if (R < 0 || R > SVOSLAM_MAX_RADIUS_CELLS) return SVOSLAM_ERR_INVALID_ARG;  // 3 R^2 fits an int32, a key fits an int64
  RegionPlan p;  // inflated by at least 1: the surface test at R = 0 reads the face neighbours
  SVO_TRY(plan_region(depth, origin, dims, R > 1 ? R : 1, &p));
  if (p.nothing) {  // no region: the entries past the end and a zero summary
    StageScope query(kStageQuery, stream);
    return init_outputs(k_max, d_chosen, d_gain, 0, nullptr, 0, d_summary, stream);
  }
  SVO_TRY(admit_region("svoslam_pool_cover_views", pool, p, R, false, stream));
  SlotRollback grown({&ws->cov_bits, &ws->cov_targets, &ws->cov_matrix, &ws->cov_state});  // what this call grows of its four slots
  StageScope query(kStageQuery, stream);
  const int rc = cover(ws, pool, depth, p, origin, R, mode, d_select, d_cands, n_cands, k_max, min_gain, d_seen, d_chosen, d_gain,
                       d_round, d_summary, stream);
  return rc == SVOSLAM_OK ? rc : grown.undo(rc, stream);
}

}  // namespace svoslam
