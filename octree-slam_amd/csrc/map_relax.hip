// map_relax.hip -- what the tiled relaxations share beyond map_relax.hpp's inline pieces: the seed kernel of
// the reach and cost fields, the finish kernel of all three fields, the tile limit, and the argument checks of the two trace
// functions.  Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): relax_seed_kernel 16 VGPRs, relax_finish_kernel
// 14, no LDS, occupancy 8, 0 bytes of scratch.
#include "map_relax.hpp"

namespace svoslam {

namespace {

__global__ __launch_bounds__(256) void relax_seed_kernel(const int32_t *__restrict__ seeds, int n, int ox, int oy, int oz, TileGrid g,
                                                         const unsigned long long *__restrict__ bits, int32_t *__restrict__ values,
                                                         int *__restrict__ flags, RelaxControl *__restrict__ ctl) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const long long x = (long long)seeds[3 * i] - ox, a = (long long)seeds[3 * i + 1] - oy, b = (long long)seeds[3 * i + 2] - oz;
  if (x < 0 || x >= g.nx || a < 0 || a >= g.na || b < 0 || b >= g.nb) return;
  if (!((bits[(a * g.ba + b * g.bb) * g.wpr + (x >> 6)] >> (x & 63)) & 1ull)) return;
  store_value(values + a * g.sa + b * g.sb + x, 0);
  atomicAdd(&ctl->seeds_used, 1);
  relax_mark_seed(flags, g, (int)x, (int)a, (int)b, (x & 63) == 0, (x & 63) == 63);
}

__global__ __launch_bounds__(256) void relax_finish_kernel(int32_t *__restrict__ values, int nx, int wpr, long long words,
                                                           const unsigned long long *__restrict__ bits) {
  const long long word = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);  // one wavefront per row word
  if (word >= words) return;
  const int lane = threadIdx.x & 63;
  const int x = (int)(word % wpr) * 64 + lane;
  if (x >= nx) return;
  const long long at = (word / wpr) * nx + x;
  const int v = values[at];
  values[at] = !((bits[word] >> lane) & 1ull) ? -2 : v == kNone ? -1 : v;
}

}  // namespace

int relax_tile_limit(const char *fn, const TileGrid &g, long long ny, long long nz) {
  if (g.tiles() * 256 > 0xFFFFFFFFll) {
    set_last_error_text("%s: %lld x %lld x %lld cells are %lld tiles, more than one launch takes (2^24 - 1)", fn, (long long)g.nx, ny, nz,
                        g.tiles());
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  return SVOSLAM_OK;
}

int relax_seed(const int32_t *d_seeds, int n_seeds, const int32_t origin[3], const TileGrid &g, const unsigned long long *bits,
               int32_t *values, int *flags, RelaxControl *ctl, hipStream_t stream) {
  if (n_seeds <= 0) return SVOSLAM_OK;
  relax_seed_kernel<<<cdiv(n_seeds, 256), 256, 0, stream>>>(d_seeds, n_seeds, origin[0], origin[1], origin[2], g, bits, values, flags, ctl);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int relax_finish(int32_t *values, long long nx, long long wpr, long long words, const unsigned long long *bits, hipStream_t stream) {
  relax_finish_kernel<<<cdiv(words, 4), 256, 0, stream>>>(values, (int)nx, (int)wpr, words, bits);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int trace_arguments(const char *fn, const int32_t *d_field, const int32_t origin[3], const int32_t dims[3], const int32_t *d_starts,
                    int32_t n_starts, int32_t max_cells, const int32_t *d_paths, const int32_t *d_lengths, bool *launch) {
  *launch = false;
  if (!origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || n_starts < 0 || max_cells < 0) return SVOSLAM_ERR_INVALID_ARG;
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  const long long plane = empty ? 0 : (long long)dims[0] * dims[1];  // below 2^62; the third factor only after it was tested
  const long long cells = plane > INT_MAX ? plane : plane * dims[2];
  if (cells > INT_MAX) {
    set_last_error_text("%s: %d x %d x %d cells are more than 2^31 - 1", fn, dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if ((long long)n_starts * max_cells > INT_MAX / 3) {
    set_last_error_text("%s: %d starts of %d cells are more than 2^31 - 1 path entries", fn, n_starts, max_cells);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_starts == 0) return SVOSLAM_OK;
  if (!d_starts || !d_lengths || (cells > 0 && !d_field) || (max_cells > 0 && !d_paths)) return SVOSLAM_ERR_INVALID_ARG;
  *launch = true;
  return SVOSLAM_OK;
}

}  // namespace svoslam
