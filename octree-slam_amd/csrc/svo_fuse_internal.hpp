// svo_fuse_internal.hpp -- what the fusion's translation units share with each other and with nobody else: svo_build.hip (kernels and host
// driver of the fusion), svo_keyrange.hip (the key-range sharded commit, which runs the driver's plan and commit on a slice of the keys),
// svo_extract.hip (the workspace's `small` buffer) and pool_state.hip (average_tile, for the re-rooting kernel).
// The __device__ helpers are the bodies the kernels of svo_build.hip were written against: `__device__ inline`, no defaulted arguments --
// a kernel's registers depend on it (DESIGN.md lesson 4).
#pragma once

#include "common.hpp"
#include "workspace.hpp"

namespace svoslam {

typedef unsigned long long u64;
typedef unsigned int u32;

// ---- planning ----------------------------------------------------------------------------------------
// number of leading 3-bit levels two distinct depth-D keys share
__device__ inline int common_levels(u64 a, u64 b, int depth) {
  const u64 x = a ^ b;  // != 0, < 2^(3D)
  const int hb = 63 - __clzll((long long)x);
  return depth - 1 - hb / 3;
}

__device__ inline bool is_head(const u64 *__restrict__ skey, int j, u64 &key, int &c, int depth) {
  key = skey[j];
  const u64 prev = j > 0 ? skey[j - 1] : 1ull;
  if (key == 1ull || key == prev) return false;
  c = (prev == 1ull) ? 0 : common_levels(key, prev, depth);
  return true;
}

__device__ inline u32 bucket_id(int p, int d) { return (u32)(p * 16 + (d - 1)); }

// averageChildren (svo.cu:384-441).  Q5: all 8 children always count.
__device__ inline u32 average_tile(const u32 *__restrict__ pool, u32 child_base) {
  const uint4 *tile = reinterpret_cast<const uint4 *>(pool + 2 * (size_t)child_base);
  u32 r = 0, g = 0, b = 0, a = 0;
#pragma unroll
  for (int q = 0; q < 4; q++) {
    const uint4 v = tile[q];
    const u32 w1a = v.y, w1b = v.w;
    r += (w1a & 0xFF) + (w1b & 0xFF);
    g += ((w1a >> 8) & 0xFF) + ((w1b >> 8) & 0xFF);
    b += ((w1a >> 16) & 0xFF) + ((w1b >> 16) & 0xFF);
    const u32 aa = w1a >> 24, ab = w1b >> 24;
    a = a > aa ? a : aa;
    a = a > ab ? a : ab;
  }
  // float sums / 8.0f of the reference are exact: integer floor division
  return (r >> 3) + ((g >> 3) << 8) + ((b >> 3) << 16) + (a << 24);
}

// ---- the asynchronous commit (fill_mip_local_kernel and the straddler kernels, svo_build.hip) ------------
constexpr u32 kNoStraddler = 0xFFFFFFFFu;

constexpr int kFillThreads = 512;  // leaves per workgroup.  Larger: fewer straddlers for the single-workgroup second launch;
// smaller: more workgroups resident next to the tracker's (which pin 150 CUs).  Measured at cfg3, fill + straddle us:
// 1024 -> 54 + 20, 512 -> 45 + 23, 256 -> 37 + 32; 2418 / 2481 / 2477 frames/s.

// layout of ws->small (u32 words): [0,256) totals | [256,513) bucket_base | [520..) PlanCounts | [640] any_valid | [648] n0 | [656] plan ticket (any_valid and the ticket start at 0 and are left at 0 by every plan)
static inline u32 *small_totals(svoslam_workspace *ws) { return ws->small.as<u32>(); }
static inline u32 *small_bucket_base(svoslam_workspace *ws) { return ws->small.as<u32>() + 256; }
static inline PlanCounts *small_counts(svoslam_workspace *ws) { return reinterpret_cast<PlanCounts *>(ws->small.as<u32>() + 520); }
static inline int *small_any(svoslam_workspace *ws) { return reinterpret_cast<int *>(ws->small.as<u32>() + 640); }
static inline u32 *small_n0(svoslam_workspace *ws) { return ws->small.as<u32>() + 648; }  // deferred commit: first new tile
static inline unsigned *small_ticket(svoslam_workspace *ws) { return ws->small.as<u32>() + 656; }  // plan_scan_finish_kernel's arrival count
static inline unsigned *small_strad_ticket(svoslam_workspace *ws) { return ws->small.as<u32>() + 664; }  // mip_straddle2_kernel's (zero between launches)

// worst-case number of split records of one call: at depth d at most min(8^d, n) distinct prefixes can be
// split (d < D), plus at most n octant-7 leaves (Q4)
static inline int64_t max_records(int n, int depth) {
  int64_t r = n;
  for (int d = 1; d < depth; d++) {
    const int64_t cells = d >= 11 ? (int64_t)1 << 62 : (int64_t)1 << (3 * d);
    r += cells < n ? cells : n;
  }
  return r;
}

// defined in svo_build.hip, launched by svo_keyrange.hip (see there)
__global__ __launch_bounds__(256) void keyrange_finish_kernel(u32 *__restrict__ pool, u32 *__restrict__ scal, unsigned long long *__restrict__ top,
                                                              int *__restrict__ d_size, int32_t *__restrict__ h_sizes, int *__restrict__ d_slot,
                                                              u32 *__restrict__ dirty);

// the commit behind svo_fuse_commit / _commit_deferred (svo_build.hip); n_live: the key-range form, see there
int commit_impl(svoslam_workspace *ws, const uint8_t *d_colors, int n, int depth, svoslam_pool *pool, bool deferred,
                hipStream_t stream, const int *n_live = nullptr);

}  // namespace svoslam
