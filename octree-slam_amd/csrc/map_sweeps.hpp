// map_sweeps.hpp -- the sweeps of a 64 x 8 x 8 tile staged in LDS that the reach field's relaxation (map_reach.hip, kStep = 1: a
// move costs a step) and the component labels' tile minimum (map_components.hip, kStep = 0) share.  Values only move between cells
// whose bit is set; each sweep is exact along its axis.  Everything is named scalars: no per-lane array.  The weighted forms below
// them are the cost field's (map_plan.hip): a move costs the weight of the cell it enters.
#pragma once
#include "common.hpp"

namespace svoslam {

// x: a wavefront per row, a lane per cell, v the cell's value ("none" where its bit of `tw` is clear).  Min-plus prefix scans up
// and down the row by doubling (k = 1, 2, .. 32); a step of k is taken only where the row word has all of the k + 1 bits from
// source to target set, so nothing passes through a cell that is not in the set.
template <int kStep>
__device__ __forceinline__ int sweep_row(int v, unsigned long long tw, int lane) {
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from below: cells lane - k .. lane all set
    const int u = __shfl_up(v, k);
    const unsigned long long run = ((2ull << k) - 1ull) << (lane >= k ? lane - k : 0);
    if (lane >= k && (tw & run) == run) v = min(v, u + k * kStep);
  }
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from above: cells lane .. lane + k
    const int u = __shfl_down(v, k);
    const unsigned long long run = ((2ull << k) - 1ull) << lane;
    if (lane + k < 64 && (tw & run) == run) v = min(v, u + k * kStep);
  }
  return v;
}

// y or z: a lane per column, serial over its 8 cells, upwards or downwards, starting from `prev` (the halo's value, or kNone) and
// restarting at every cell whose bit is clear.  Cell c is at cells[c * kPitch], its row word at words[c * kWordPitch].  Returns
// 1 if a cell was lowered, else 0.
template <int kStep, int kNone, int kPitch, int kWordPitch, bool kUp>
__device__ __forceinline__ int sweep_column(int32_t *cells, const unsigned long long *words, int lane, int prev) {
  int lowered = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = kUp ? i : 7 - i;
    if ((words[c * kWordPitch] >> lane) & 1ull) {
      const int v = cells[c * kPitch];
      prev = min(v, prev + kStep);
      if (prev < v) { cells[c * kPitch] = prev; lowered = 1; }
    } else {
      prev = kNone;
    }
  }
  return lowered;
}

// The weighted forms (map_plan.hip): entering a cell costs its own weight wt >= 1, so a tile needs the weights of its own cells only.
//
// x: v the cell's cost ("none" = kNone where its bit of `tw` is clear or nothing has reached it), wt its weight (0 where the bit is
// clear).  With P the inclusive and E = P - wt the exclusive prefix sum of the row's weights, going up the row s(q) = P(q) + min
// over p <= q of the same run of (s(p) - P(p)), going down s(q) = min over p >= q of the run of (s(p) + E(p)) - E(q): two plain
// minimum scans by the doubling and the run-mask test of sweep_row.  The term p = q is v itself, so the result never exceeds v, and
// a term that starts from kNone gives kNone or more: with costs below kNone "none" stays "none".  64 weights of 16 bits sum to
// less than 2^22, so kNone = 2^30 leaves room on both sides.
__device__ __forceinline__ int sweep_row_weighted(int v, int wt, unsigned long long tw, int lane) {
  int P = wt;  // the inclusive prefix sum of the weights, over all 64 lanes: only differences inside a run are used
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {
    const int u = __shfl_up(P, k);
    if (lane >= k) P += u;
  }
  int a = v - P;
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from below: cells lane - k .. lane all set
    const int u = __shfl_up(a, k);
    const unsigned long long run = ((2ull << k) - 1ull) << (lane >= k ? lane - k : 0);
    if (lane >= k && (tw & run) == run) a = min(a, u);
  }
  v = a + P;
  const int E = P - wt;
  int b = v + E;
#pragma unroll
  for (int k = 1; k < 64; k *= 2) {  // from above: cells lane .. lane + k
    const int u = __shfl_down(b, k);
    const unsigned long long run = ((2ull << k) - 1ull) << lane;
    if (lane + k < 64 && (tw & run) == run) b = min(b, u);
  }
  return b - E;
}

// y or z: sweep_column with the cell's own weight, at weights[c * kWeightPitch], in place of kStep
template <int kNone, int kPitch, int kWordPitch, int kWeightPitch, bool kUp>
__device__ __forceinline__ int sweep_column_weighted(int32_t *cells, const unsigned long long *words, const uint16_t *weights, int lane,
                                                     int prev) {
  int lowered = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    const int c = kUp ? i : 7 - i;
    if ((words[c * kWordPitch] >> lane) & 1ull) {
      const int v = cells[c * kPitch];
      prev = min(v, prev + (int)weights[c * kWeightPitch]);
      if (prev < v) { cells[c * kPitch] = prev; lowered = 1; }
    } else {
      prev = kNone;
    }
  }
  return lowered;
}

}  // namespace svoslam
