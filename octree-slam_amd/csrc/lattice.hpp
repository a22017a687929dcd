// lattice.hpp -- the 2^d lattice the surface mesh is built on and the map queries walk (DESIGN.md sections 12 - 15): one
// definition of its planes and of the cell of a coordinate for map_query.hip and map_volume.hip, and, on the host, for
// svoslam_box_to_cells (map_field.hip; the host is compiled without contraction too: the same binary32 operations)
#pragma once
#include "common.hpp"

namespace svoslam {

// plane k (0..N) of one axis of the 2^d lattice: the surface mesh's vertex coordinate (svo_surface.hip: weld_scatter_kernel)
__host__ __device__ inline float lattice_plane(float c, int k, int N, float h) { return c + (float)(2 * k - N) * h; }

// lo + the number of k in lo+1 .. lo+size-1 whose plane is <= p (< p when `strict`): the cell of p among the `size` cells (a
// power of two) that start at lo.  Planes ascend with k, so the count is found by probing; a NaN counts nothing.
__host__ __device__ inline int cell_in_block(float c, int N, float h, float p, int lo, int size, bool strict) {
  int k = lo;
  for (int s = size >> 1; s > 0; s >>= 1) {
    const float pl = lattice_plane(c, k + s, N, h);
    if (strict ? pl < p : pl <= p) k += s;
  }
  return k;
}

}  // namespace svoslam
