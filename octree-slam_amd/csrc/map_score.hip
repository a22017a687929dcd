// map_score.hip -- scoring candidate poses against a distance field of a map region (own specification; the
// restatement the device must equal bit for bit is tests/test_score_cpu.py): for P poses and n sensor points, every point moved by
// every pose (mat4_mul_point, the one definition of a pose applied to a point), its cell found on the lattice (cell_in_block, the
// one definition of the cell of a coordinate), the field read there, and per pose the sum of the values and three counts.  The
// sums are integers, so lanes, wavefronts and workgroups combine them in any order and the result is still exact.
//
//   score_kernel<false>  the whole-pose form, for many poses: one workgroup per pose, 256 lanes stride over the n points.  The pose
//                        is read through a uniform index (16 scalar loads, SGPRs); the points are re-read by every workgroup, from
//                        L2 (n = 4800 is 56 KB).  Per pair three cell searches of d dependent probes each, then ONE gather from the
//                        field, the only irregular access.  A shuffle reduction per wavefront, 4 partial records through LDS,
//                        and lane 0 writes the pose's outputs directly: no atomics, no second launch unless d_best is wanted.
//   score_kernel<true>   the split form, for few poses of many points: workgroup (chunk, pose) takes kChunk points of one pose and
//                        adds its partial record to the pose's record in the workspace with integer atomics (one lane per
//                        workgroup: 4 atomics per 1024 pairs).  zero_kernel clears the records before it.
//   finish_kernel        one workgroup over the records: cost = sum + miss_cost * (far + outside); writes the per-pose outputs (split
//                        form) and the best (cost, index) among the poses with near >= min_near, the lowest index among equal costs.
// The host chooses the form from (n, n_poses): split iff n > kChunk and n_poses < kSplitBelow.
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): see DESIGN.md section 20; no scratch in any kernel, LDS 96
// bytes (score_kernel) and 64 bytes (finish_kernel).  No per-lane arrays indexed at run time; every store is a vector store from plain C++.
#include <limits.h>

#include "lattice.hpp"
#include "map_score.hpp"
#include "stage_timing.hpp"
#include "workspace.hpp"

namespace svoslam {

namespace {

constexpr int kChunk = 1024;       // points per workgroup in the split form: 4 per lane
constexpr int kSplitBelow = 512;   // the split form is for fewer poses than this: with more, one workgroup per pose fills the device

struct ScoreRec {  // what one pose's pairs add up to
  unsigned long long sum;  // of the field's values over the NEAR pairs
  int near, far, outside, pad;
};

template <bool SPLIT>
__global__ __launch_bounds__(256) void score_kernel(const int32_t *__restrict__ field, int N, float cx, float cy, float cz, float h, int ox,
                                                    int oy, int oz, int nx, int ny, int nz, const float *__restrict__ points, int n,
                                                    const float *__restrict__ poses, int chunks, long long miss,
                                                    ScoreRec *__restrict__ rec, long long *__restrict__ out_cost,
                                                    int32_t *__restrict__ out_near, int32_t *__restrict__ out_far,
                                                    int32_t *__restrict__ out_outside) {
  const int pose = SPLIT ? (int)(blockIdx.x / (unsigned)chunks) : (int)blockIdx.x;
  const int first = SPLIT ? (int)(blockIdx.x % (unsigned)chunks) * kChunk : 0;
  const int last = SPLIT ? (n - first < kChunk ? n : first + kChunk) : n;
  const float *__restrict__ m = poses + 16 * (size_t)pose;  // uniform: scalar loads
  const float c[3] = {cx, cy, cz};
  float lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    lo[a] = lattice_plane(c[a], 0, N, h);
    hi[a] = lattice_plane(c[a], N, N, h);
  }
  unsigned long long sum = 0ull;
  int near = 0, far = 0, outside = 0;
  for (int i = first + (int)threadIdx.x; i < last; i += 256) {
    const float px = points[3 * (size_t)i], py = points[3 * (size_t)i + 1], pz = points[3 * (size_t)i + 2];
    if (!(finitef_(px) && finitef_(py) && finitef_(pz))) continue;  // void: counts nowhere
    float w[3];
    mat4_mul_point(m, px, py, pz, 1.0f, w[0], w[1], w[2]);
    bool inside = finitef_(w[0]) && finitef_(w[1]) && finitef_(w[2]);
    int q[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      inside = inside && lo[a] <= w[a] && w[a] <= hi[a];
      q[a] = cell_in_block(c[a], N, h, w[a], 0, N, false);
    }
    const unsigned rx = (unsigned)(q[0] - ox), ry = (unsigned)(q[1] - oy), rz = (unsigned)(q[2] - oz);
    inside = inside && rx < (unsigned)nx && ry < (unsigned)ny && rz < (unsigned)nz;
    if (inside) {  // the index is below nx * ny * nz <= 2^31 - 1
      const int v = field[((size_t)rz * (unsigned)ny + ry) * (unsigned)nx + rx];
      if (v >= 0) {
        sum += (unsigned)v;
        near++;
      } else {
        far++;
      }
    } else {
      outside++;
    }
  }
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    sum += __shfl_xor(sum, s);
    near += __shfl_xor(near, s);
    far += __shfl_xor(far, s);
    outside += __shfl_xor(outside, s);
  }
  __shared__ ScoreRec part[4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    part[wave].sum = sum;
    part[wave].near = near;
    part[wave].far = far;
    part[wave].outside = outside;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < 4; k++) {
    sum += part[k].sum;
    near += part[k].near;
    far += part[k].far;
    outside += part[k].outside;
  }
  if (SPLIT) {  // the records were cleared by zero_kernel; finish_kernel reads them after this launch
    atomicAdd(&rec[pose].sum, sum);
    atomicAdd(&rec[pose].near, near);
    atomicAdd(&rec[pose].far, far);
    atomicAdd(&rec[pose].outside, outside);
  } else {
    if (rec) {
      rec[pose].sum = sum;
      rec[pose].near = near;
      rec[pose].far = far;
      rec[pose].outside = outside;
    }
    if (out_cost) out_cost[pose] = (long long)sum + miss * ((long long)far + outside);
    if (out_near) out_near[pose] = near;
    if (out_far) out_far[pose] = far;
    if (out_outside) out_outside[pose] = outside;
  }
}

__global__ __launch_bounds__(256) void zero_kernel(unsigned long long *__restrict__ words, unsigned count) {
  const unsigned i = blockIdx.x * 256u + threadIdx.x;
  if (i < count) words[i] = 0ull;
}

// one workgroup.  write_outputs: the split form, whose per-pose outputs are still to be written from the records
__global__ __launch_bounds__(256) void finish_kernel(const ScoreRec *__restrict__ rec, int n_poses, long long miss, int min_near,
                                                     bool write_outputs, long long *__restrict__ out_cost,
                                                     int32_t *__restrict__ out_near, int32_t *__restrict__ out_far,
                                                     int32_t *__restrict__ out_outside, long long *__restrict__ out_best) {
  long long best = LLONG_MAX, best_at = -1;  // a cost stays below 2^62
  for (int p = threadIdx.x; p < n_poses; p += 256) {
    const ScoreRec r = rec[p];
    const long long cost = (long long)r.sum + miss * ((long long)r.far + r.outside);
    if (write_outputs) {
      if (out_cost) out_cost[p] = cost;
      if (out_near) out_near[p] = r.near;
      if (out_far) out_far[p] = r.far;
      if (out_outside) out_outside[p] = r.outside;
    }
    if (r.near >= min_near && cost < best) {  // p ascends: the first of equal costs stays
      best = cost;
      best_at = p;
    }
  }
  if (!out_best) return;  // uniform
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) {
    const long long other = __shfl_xor(best, s), other_at = __shfl_xor(best_at, s);
    if (other_at >= 0 && (best_at < 0 || other < best || (other == best && other_at < best_at))) {
      best = other;
      best_at = other_at;
    }
  }
  __shared__ long long part[4][2];
  if ((threadIdx.x & 63) == 0) {
    part[threadIdx.x >> 6][0] = best;
    part[threadIdx.x >> 6][1] = best_at;
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < 4; k++) {
    const long long other = part[k][0], other_at = part[k][1];
    if (other_at >= 0 && (best_at < 0 || other < best || (other == best && other_at < best_at))) {
      best = other;
      best_at = other_at;
    }
  }
  out_best[0] = best_at >= 0 ? best : -1;
  out_best[1] = best_at;
}

}  // namespace

int score_poses(svoslam_workspace *ws, const int32_t *d_dist2, int depth, const float center[3], float edge, const int32_t origin[3],
                const int32_t dims[3], const float *d_points, int32_t n, const float *d_poses, int32_t n_poses, int32_t miss_cost,
                int32_t min_near, int64_t *d_cost, int32_t *d_near, int32_t *d_far, int32_t *d_outside, int64_t *d_best,
                hipStream_t stream) {
  if (!ws || !center || !origin || !dims || depth < 1 || depth > SVOSLAM_MAX_DEPTH || !(edge > 0.0f)) return SVOSLAM_ERR_INVALID_ARG;
  const long long N = 1ll << depth;
  long long cells = 1;  // every side is <= 2^16: no overflow
  for (int a = 0; a < 3; a++) {
    if (dims[a] < 0 || origin[a] < 0 || (long long)origin[a] + dims[a] > N) return SVOSLAM_ERR_INVALID_ARG;
    cells *= dims[a];
  }
  if (n < 0 || n_poses < 0 || miss_cost < 0 || miss_cost > SVOSLAM_MAX_MISS_COST || min_near < 0) return SVOSLAM_ERR_INVALID_ARG;
  if ((n > 0 && !d_points) || (n_poses > 0 && !d_poses)) return SVOSLAM_ERR_INVALID_ARG;
  if (cells > 0 && n > 0 && n_poses > 0 && !d_dist2) return SVOSLAM_ERR_INVALID_ARG;
  if (n_poses > 0 && !d_cost && !d_near && !d_far && !d_outside && !d_best) return SVOSLAM_ERR_INVALID_ARG;
  if (cells > (long long)INT_MAX) {
    set_last_error_text("svoslam_score_poses: %d x %d x %d cells are more than 2^31 - 1", dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_poses == 0 && !d_best) return SVOSLAM_OK;
  const long long chunks = ((long long)n + kChunk - 1) / kChunk;
  const bool split = n > kChunk && n_poses < kSplitBelow;  // chunks * n_poses then stays below 2^21 * 2^9
  ScoreRec *rec = nullptr;
  if (n_poses > 0 && (split || d_best)) {
    const int rc = ws->score_rec.reserve((size_t)n_poses * sizeof(ScoreRec));
    if (rc != SVOSLAM_OK) {  // nothing the call allocated stays behind
      ws->score_rec.release();
      return rc;
    }
    rec = ws->score_rec.as<ScoreRec>();
  }
  long long *cost = reinterpret_cast<long long *>(d_cost), *best = reinterpret_cast<long long *>(d_best);
  const float h = edge / (float)(1 << depth);
  StageScope query(kStageQuery, stream);
  if (n_poses > 0) {
    if (split) {
      const unsigned words = (unsigned)n_poses * (unsigned)(sizeof(ScoreRec) / 8);
      zero_kernel<<<cdiv(words, 256), 256, 0, stream>>>(reinterpret_cast<unsigned long long *>(rec), words);
      SVO_LAUNCH_CHECK();
      score_kernel<true><<<(unsigned)(chunks * n_poses), 256, 0, stream>>>(d_dist2, (int)N, center[0], center[1], center[2], h, origin[0],
                                                                         origin[1], origin[2], dims[0], dims[1], dims[2], d_points, n,
                                                                         d_poses, (int)chunks, (long long)miss_cost, rec, nullptr, nullptr,
                                                                         nullptr, nullptr);
    } else {
      score_kernel<false><<<(unsigned)n_poses, 256, 0, stream>>>(d_dist2, (int)N, center[0], center[1], center[2], h, origin[0], origin[1],
                                                                origin[2], dims[0], dims[1], dims[2], d_points, n, d_poses, 1,
                                                                (long long)miss_cost, d_best ? rec : nullptr, cost, d_near, d_far,
                                                                d_outside);
    }
    SVO_LAUNCH_CHECK();
  }
  if (split || d_best) {
    finish_kernel<<<1, 256, 0, stream>>>(rec, n_poses, (long long)miss_cost, min_near, split, cost, d_near, d_far, d_outside, best);
    SVO_LAUNCH_CHECK();
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
