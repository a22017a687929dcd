// map_descend.hpp -- what the volume queries (map_volume.hip) and the region fields' raster (map_region.hip) share: the Morton
// code of a cell (x lowest: the pool's octant order) and one descent from the root along a cell's path
#pragma once
#include "common.hpp"

namespace svoslam {

// bit i of v (i < 16) moved to bit 3i, and back
__device__ inline unsigned long long spread3(uint32_t v) {
  unsigned long long x = v & 0xFFFFull;
  x = (x | (x << 16)) & 0x0000FF0000FFull;
  x = (x | (x << 8)) & 0x00F00F00F00Full;
  x = (x | (x << 4)) & 0x0C30C30C30C3ull;
  x = (x | (x << 2)) & 0x249249249249ull;
  return x;
}
__device__ inline int compact3(unsigned long long m) {
  unsigned long long x = m & 0x249249249249ull;
  x = (x | (x >> 2)) & 0x0C30C30C30C3ull;
  x = (x | (x >> 4)) & 0x00F00F00F00Full;
  x = (x | (x >> 8)) & 0x0000FF0000FFull;
  x = (x | (x >> 16)) & 0xFFFFull;
  return (int)x;
}
__device__ inline unsigned long long morton3(int x, int y, int z) {
  return spread3((uint32_t)x) | (spread3((uint32_t)y) << 1) | (spread3((uint32_t)z) << 2);
}

// the distance in cells, on one axis, from q to the block of 2^sh cells around x
__device__ inline int axis_gap(int x, int sh, int q) {
  const int lo = (x >> sh) << sh, hi = lo + (1 << sh) - 1;
  return q < lo ? lo - q : (q > hi ? q - hi : 0);
}

// One descent from the root along the path of cell (x, y, z) = m.  Returns the level l it ended at: the block of level l around
// the cell is free (or, with kPrune, not nearer to q than `best`), unless `hit`: then l == d and the cell is occupied, nd its
// node and w its words.
template <bool kPrune>
__device__ inline int descend(const uint32_t *__restrict__ pool, unsigned long long m, int d, int x, int y, int z, int qx, int qy,
                              int qz, int best, uint32_t &nd, uint2 &w, bool &hit) {
  uint32_t child = 0u;
  int l = 1;
  hit = false;
  for (;; l++) {
    const int sh = d - l;
    if (kPrune) {
      const int gx = axis_gap(x, sh, qx), gy = axis_gap(y, sh, qy), gz = axis_gap(z, sh, qz);
      if (gx * gx + gy * gy + gz * gz >= best) break;
    }
    nd = child + (uint32_t)((m >> (3 * sh)) & 7ull);
    w = *reinterpret_cast<const uint2 *>(pool + 2 * (size_t)nd);
    if ((w.y >> 24) <= 127u) break;
    if (l == d) { hit = true; break; }
    if (!(w.x & kFlag)) break;
    child = w.x & kMask;
  }
  return l;
}

}  // namespace svoslam
