// supercover_walk.hpp -- the integer supercover walk of DESIGN.md section 19 as a function with a per-cell functor (section 22).
// map_visibility.hip's sight_kernel keeps its own copy of the loop: its generated code is recorded in section 19.
//
// From cell a towards cell b = a + D the walk calls visit(x, y, z) for every cell of S(a, b) -- the cells other than a and b whose
// closed cube meets the closed centre-to-centre segment -- each exactly once and never for a or b, in this order: crossing by
// crossing from a; where two or three axes cross at the same parameter (the segment passes through an edge or a corner) first the
// side cells of one axis in x, y, z order, then those of two axes (xy, xz, yz), then the diagonal cell.  That is the order
// tests/test_visibility_cpu.py::walk_cells lists them in and sight_kernel tests them in.  visit returns true to end the walk.
//
// Keys.  Axis a has made i_a of its n_a = |D_a| crossings; its next one is at the parameter (2 i_a + 1) / (2 n_a).  With P_a the
// product of the other two n, a zero taken as 1, the key (2 i_a + 1) * P_a orders the parameters exactly (all three are the
// parameters times 2 * m_x * m_y * m_z, m = max(n, 1)), grows by 2 P_a per crossing, and an axis that has made all its crossings
// holds (2 n_a + 1) * P_a, a parameter above 1 and so above every live axis's.  An axis with n_a = 0 has the key "never".
//   Bound: i_a <= n_a, so a key is at most (2 n_a + 1) * P_a <= (2 n + 1) * n^2 for n = the largest |D|.  Section 19 had n <= 4096
//   (keys below 2^38).  Here n is bounded by the region alone when both ends lie in it: with at most 2^16 cells per axis n <= 2^16
//   - 1, 2 n + 1 < 2^17, P_a < 2^32, and every key is below 2^49, under "never" = 2^62 in an int64.  An end outside the region can
//   be anywhere in int32: n < 2^32, keys below 2^33 * 2^64 = 2^97, under "never" = 2^126 in a 128-bit integer; the caller chooses
//   the key type by n (walk_fits_int64).
// Termination: every pass makes at least one crossing and there are n_x + n_y + n_z of them.
#pragma once
#include <stdint.h>

#ifndef __host__
#define __host__
#define __device__
#endif

namespace svoslam {

constexpr long long kWalkMaxAxisCells = 1ll << 16;  // a region's cells per axis for which int64 keys are proven

template <class K> struct WalkNever;
template <> struct WalkNever<long long> { static constexpr long long value = 1ll << 62; };
template <> struct WalkNever<__int128> { static constexpr __int128 value = (__int128)1 << 126; };

// |D| per axis for which the int64 keys stay below 2^49
__host__ __device__ inline bool walk_fits_int64(long long nx, long long ny, long long nz) {
  return nx < kWalkMaxAxisCells && ny < kWalkMaxAxisCells && nz < kWalkMaxAxisCells;
}

// (cx, cy, cz): cell a in the caller's coordinates; (dx, dy, dz) = b - a.  The cells handed to visit are a plus whole steps, so
// they stay in the bounding box of a and b.  -> true iff visit ended the walk.
template <class K, class Visit>
__host__ __device__ inline bool supercover_walk(int cx, int cy, int cz, long long dx, long long dy, long long dz, Visit &&visit) {
  const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
  if (!(ax | ay | az)) return false;
  const int sx = dx < 0 ? -1 : 1, sy = dy < 0 ? -1 : 1, sz = dz < 0 ? -1 : 1;
  const K mx = ax ? ax : 1, my = ay ? ay : 1, mz = az ? az : 1;
  const K gx = 2 * my * mz, gy = 2 * mx * mz, gz = 2 * mx * my;  // what a key grows by per crossing
  K kx = ax ? my * mz : WalkNever<K>::value, ky = ay ? mx * mz : WalkNever<K>::value, kz = az ? mx * my : WalkNever<K>::value;
  long long left = ax + ay + az;  // crossings still to make
  for (;;) {
    const K kyz = ky < kz ? ky : kz;
    const K first = kx < kyz ? kx : kyz;
    const bool bx = kx == first, by = ky == first, bz = kz == first;
    const int ex = bx ? sx : 0, ey = by ? sy : 0, ez = bz ? sz : 0;
    const int crossing = (int)bx + (int)by + (int)bz;
    left -= crossing;
    if (crossing > 1) {  // through an edge or a corner: the cells beside the diagonal step
      if (bx && visit(cx + ex, cy, cz)) return true;
      if (by && visit(cx, cy + ey, cz)) return true;
      if (bz && visit(cx, cy, cz + ez)) return true;
      if (crossing == 3 && (visit(cx + ex, cy + ey, cz) || visit(cx + ex, cy, cz + ez) || visit(cx, cy + ey, cz + ez))) return true;
    }
    cx += ex; cy += ey; cz += ez;
    if (bx) kx += gx;
    if (by) ky += gy;
    if (bz) kz += gz;
    if (left == 0) return false;  // arrived at b: not visited
    if (visit(cx, cy, cz)) return true;
  }
}

}  // namespace svoslam
