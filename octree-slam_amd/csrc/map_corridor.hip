// map_corridor.hip -- safe corridors along planned paths: axis-aligned boxes of free cells grown layer by layer over a distance field,
// and the chain of overlapping boxes that holds a path (own specification, include/svoslam_corridor.h and DESIGN.md section 27: the
// reference has nothing like it; the restatements the device must equal value for value are in tests/test_corridor_cpu.py).  Both
// calls read a distance field as svoslam_pool_distance_field writes it and take no pool and no workspace.  g(c) is map_paths.hip's:
// the field's value at c, +infinity where it is -1, 0 for a cell outside the region; a cell is free iff g > r^2.
//
//   slab_free             the test behind every layer: an O(1) bounds test of the slab against the region first (a slab that leaves
//                         it holds a cell that is not free, and nothing outside the region is read), then the 64 lanes stride over
//                         the slab's cells in batches, x fastest, so a slab that spans x is read in coalesced rows; a __ballot after
//                         each batch ends the test at the first batch that holds a cell that is not free.
//   grow                  the rounds of the specification, wave-uniform: -x +x -y +y -z +z, each direction against the box as the
//                         directions before it left it, until a round grows nothing.  The box and the six layer counts are scalars.
//   grow_boxes_kernel     one wavefront per seed: validity (lo <= hi, inside the region in 64 bits, every cell free by slab_free over
//                         the seed itself), then grow.
//   path_corridors_kernel one wavefront per path, the anchor a uniform.  The seed is p_a, with p_(a+1) when that is a free face
//                         neighbour; e(a) tests the following path cells 64 per batch, one per lane, and the first lane outside the
//                         box (or beyond the path) is found by ballot and count-trailing-zeros.
// Every device loop ends by its own data.  A direction grows at most E layers, so a grow makes at most 6E growing rounds and one more
// that grows nothing: at most 6E + 6 direction tries beyond the growing ones; a box that has reached the region's border fails the
// bounds test at once, so the rounds are also bounded by the region's extent.  A slab is at most the region (2^31 - 1 cells), its
// batch loop runs to its end or leaves earlier.  The anchor rises strictly and stays below L; the batch loop of e(a) ends at the
// latest in the batch that reaches L, whose lanes beyond the path count as outside.
//
// Resource report (hipcc -Rpass-analysis=kernel-resource-usage, gfx950): grow_boxes_kernel 13 VGPRs / 69 SGPRs, occupancy 8;
// path_corridors_kernel 40 VGPRs / 91 SGPRs, occupancy 8; both 0 bytes of scratch, no LDS.  No per-lane arrays indexed at run time, no
// inline assembly, plain vector stores.
#include <limits.h>

#include "map_corridor.hpp"
#include "stage_timing.hpp"

namespace svoslam {

namespace {

constexpr long long kMaxAxisCells = 1ll << 16;  // a region's cells per axis, the limit svoslam_field_shorten_paths has

struct FieldView {  // the region's field; a cell is addressed relative to the region's first cell
  const int32_t *__restrict__ dist2;
  int nx, ny, nz;
  // g of a cell given relative to the region, as map_paths.hip has it: nothing outside the region is read
  __device__ __forceinline__ int g(long long x, long long y, long long z) const {
    if (x < 0 || x >= nx || y < 0 || y >= ny || z < 0 || z >= nz) return 0;
    const int v = dist2[(z * ny + y) * nx + x];
    return v < 0 ? INT_MAX : v;
  }
};

struct Box {  // relative to the region's first cell, inclusive; wave-uniform
  int lx, ly, lz, hx, hy, hz;
};

// every cell of the slab lo .. hi (lo <= hi on every axis) is free
__device__ __forceinline__ bool slab_free(const FieldView &f, int r2, int lane, int lx, int ly, int lz, int hx, int hy, int hz) {
  if (lx < 0 || ly < 0 || lz < 0 || hx >= f.nx || hy >= f.ny || hz >= f.nz) return false;  // a cell outside the region is not free
  const unsigned sx = hx - lx + 1, sy = hy - ly + 1, sz = hz - lz + 1;
  const unsigned count = sx * sy * sz;  // at most the region: 2^31 - 1
  for (unsigned base = 0; base < count; base += 64) {  // base <= 2^31: the sum does not wrap
    const unsigned idx = base + lane;
    bool blocked = false;
    if (idx < count) {
      const unsigned row = idx / sx;
      const long long x = lx + (int)(idx - row * sx), y = ly + (int)(row % sy), z = lz + (int)(row / sy);
      const int v = f.dist2[(z * f.ny + y) * f.nx + x];
      blocked = v >= 0 && v <= r2;
    }
    if (__ballot(blocked)) return false;
  }
  return true;
}

// grow(box) of the specification; -> the layers added
__device__ __forceinline__ int grow(const FieldView &f, int r2, int E, int lane, Box &b) {
  int g0 = 0, g1 = 0, g2 = 0, g3 = 0, g4 = 0, g5 = 0;
  // one direction: the slab beside the face, against the box as it is now
  auto attempt = [&](int &grown, int &face, int step, int lx, int ly, int lz, int hx, int hy, int hz) {
    if (grown >= E || !slab_free(f, r2, lane, lx, ly, lz, hx, hy, hz)) return false;
    face += step;
    grown++;
    return true;
  };
  bool any = true;
  while (any) {  // at most 6E rounds grow
    any = attempt(g0, b.lx, -1, b.lx - 1, b.ly, b.lz, b.lx - 1, b.hy, b.hz);
    any |= attempt(g1, b.hx, +1, b.hx + 1, b.ly, b.lz, b.hx + 1, b.hy, b.hz);
    any |= attempt(g2, b.ly, -1, b.lx, b.ly - 1, b.lz, b.hx, b.ly - 1, b.hz);
    any |= attempt(g3, b.hy, +1, b.lx, b.hy + 1, b.lz, b.hx, b.hy + 1, b.hz);
    any |= attempt(g4, b.lz, -1, b.lx, b.ly, b.lz - 1, b.hx, b.hy, b.lz - 1);
    any |= attempt(g5, b.hz, +1, b.lx, b.ly, b.hz + 1, b.hx, b.hy, b.hz + 1);
  }
  return g0 + g1 + g2 + g3 + g4 + g5;
}

__device__ __forceinline__ void store_box(int32_t *__restrict__ out, const Box &b, int ox, int oy, int oz) {
  out[0] = b.lx + ox; out[1] = b.ly + oy; out[2] = b.lz + oz;
  out[3] = b.hx + ox; out[4] = b.hy + oy; out[5] = b.hz + oz;
}

__global__ __launch_bounds__(256) void grow_boxes_kernel(FieldView f, int ox, int oy, int oz, int r2, int E, const int32_t *__restrict__ seeds,
                                                         int n, int32_t *__restrict__ boxes, int32_t *__restrict__ layers) {
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // n <= 2^31 - 1, compared unsigned
  if (wave >= (unsigned)n) return;
  const int lane = threadIdx.x & 63;
  const int32_t *__restrict__ seed = seeds + 6ll * wave;
  int32_t *__restrict__ out = boxes + 6ll * wave;
  const int s0 = __builtin_amdgcn_readfirstlane(seed[0]), s1 = __builtin_amdgcn_readfirstlane(seed[1]),
            s2 = __builtin_amdgcn_readfirstlane(seed[2]), s3 = __builtin_amdgcn_readfirstlane(seed[3]),
            s4 = __builtin_amdgcn_readfirstlane(seed[4]), s5 = __builtin_amdgcn_readfirstlane(seed[5]);
  const long long lx = (long long)s0 - ox, ly = (long long)s1 - oy, lz = (long long)s2 - oz;
  const long long hx = (long long)s3 - ox, hy = (long long)s4 - oy, hz = (long long)s5 - oz;
  int added = -1;
  // lo <= hi and inside the region, in 64 bits; then the six fit an int and slab_free may read every cell
  if (lx >= 0 && ly >= 0 && lz >= 0 && lx <= hx && ly <= hy && lz <= hz && hx < f.nx && hy < f.ny && hz < f.nz &&
      slab_free(f, r2, lane, (int)lx, (int)ly, (int)lz, (int)hx, (int)hy, (int)hz)) {
    Box b = {(int)lx, (int)ly, (int)lz, (int)hx, (int)hy, (int)hz};
    added = grow(f, r2, E, lane, b);
    if (lane == 0) store_box(out, b, ox, oy, oz);
  } else if (lane == 0) {
    out[0] = s0; out[1] = s1; out[2] = s2; out[3] = s3; out[4] = s4; out[5] = s5;
  }
  if (lane == 0) layers[wave] = added;
}

__global__ __launch_bounds__(256) void path_corridors_kernel(FieldView f, int ox, int oy, int oz, int r2, int E,
                                                             const int32_t *__restrict__ paths, const int32_t *__restrict__ lengths,
                                                             int n_paths, int max_cells, int max_boxes, int32_t *__restrict__ boxes,
                                                             int32_t *__restrict__ anchors, int32_t *__restrict__ counts,
                                                             int32_t *__restrict__ gaps) {
  const unsigned wave = __builtin_amdgcn_readfirstlane(blockIdx.x * 4u + (threadIdx.x >> 6));  // n_paths <= 2^31 - 1, compared unsigned
  if (wave >= (unsigned)n_paths) return;
  const int lane = threadIdx.x & 63;
  const long long stored = __builtin_amdgcn_readfirstlane(lengths[wave]);
  const int L = (int)min(stored < 0 ? -stored : stored, (long long)max_cells);
  const int32_t *__restrict__ cells = paths + (long long)wave * max_cells * 3;
  int32_t *__restrict__ out_boxes = boxes + (long long)wave * max_boxes * 6;
  int32_t *__restrict__ out_anchors = anchors + (long long)wave * max_boxes;
  int count = 0, broken = 0;
  if (L > 0) {
    int a = 0;
    while (true) {  // a rises by at least 1 per pass and the pass with e == L - 1 is the last
      const int px = __builtin_amdgcn_readfirstlane(cells[3 * a]), py = __builtin_amdgcn_readfirstlane(cells[3 * a + 1]),
                pz = __builtin_amdgcn_readfirstlane(cells[3 * a + 2]);
      const long long rx = (long long)px - ox, ry = (long long)py - oy, rz = (long long)pz - oz;
      const bool empty = f.g(rx, ry, rz) <= r2;
      int e = a;
      if (!empty) {  // free: p_a lies in the region, rx, ry, rz are below 2^16
        Box b = {(int)rx, (int)ry, (int)rz, (int)rx, (int)ry, (int)rz};
        if (a + 1 < L) {
          const int qx = __builtin_amdgcn_readfirstlane(cells[3 * a + 3]), qy = __builtin_amdgcn_readfirstlane(cells[3 * a + 4]),
                    qz = __builtin_amdgcn_readfirstlane(cells[3 * a + 5]);
          const long long dx = (long long)qx - px, dy = (long long)qy - py, dz = (long long)qz - pz;
          const long long ax = dx < 0 ? -dx : dx, ay = dy < 0 ? -dy : dy, az = dz < 0 ? -dz : dz;
          if (ax + ay + az == 1 && f.g(rx + dx, ry + dy, rz + dz) > r2) {  // a free face neighbour: the seed is the pair
            b.lx += min((int)dx, 0); b.ly += min((int)dy, 0); b.lz += min((int)dz, 0);
            b.hx += max((int)dx, 0); b.hy += max((int)dy, 0); b.hz += max((int)dz, 0);
          }
        }
        grow(f, r2, E, lane, b);
        for (int base = a + 1;; base += 64) {  // base + 63 < 2^31: L * 3 <= 2^31 - 1; ends in the batch that reaches L at the latest
          const int j = base + lane;
          bool outside = true;  // a lane beyond the path counts as outside
          if (j < L) {
            const long long qx = (long long)cells[3 * j] - ox, qy = (long long)cells[3 * j + 1] - oy, qz = (long long)cells[3 * j + 2] - oz;
            outside = qx < b.lx || qx > b.hx || qy < b.ly || qy > b.hy || qz < b.lz || qz > b.hz;
          }
          const unsigned long long out_mask = __ballot(outside);
          if (out_mask) {
            e = base + __builtin_ctzll(out_mask) - 1;
            break;
          }
        }
        if (lane == 0 && count < max_boxes) store_box(out_boxes + 6ll * count, b, ox, oy, oz);
      } else if (lane == 0 && count < max_boxes) {  // the empty box: lo = p_a, hi = p_a - 1 in int32 arithmetic
        int32_t *__restrict__ o = out_boxes + 6ll * count;
        o[0] = px; o[1] = py; o[2] = pz;
        o[3] = (int)((unsigned)px - 1u); o[4] = (int)((unsigned)py - 1u); o[5] = (int)((unsigned)pz - 1u);
      }
      if (lane == 0 && count < max_boxes) out_anchors[count] = a;
      count++;
      if (empty || (e == a && a < L - 1)) broken++;
      if (e == L - 1) break;
      a = e > a ? e : a + 1;
    }
  }
  if (lane == 0) {
    counts[wave] = count;
    if (gaps) gaps[wave] = broken;
  }
}

// the checks both calls share: the region's size.  -> SVOSLAM_OK with *cells set
int region_cells(const char *who, const int32_t dims[3], long long *cells) {
  const bool empty = dims[0] == 0 || dims[1] == 0 || dims[2] == 0;
  const long long plane = empty ? 0 : (long long)dims[0] * dims[1];  // below 2^62; the third factor only after it was tested
  *cells = plane > INT_MAX ? plane : plane * dims[2];
  if (*cells > INT_MAX) {
    set_last_error_text("%s: %d x %d x %d cells are more than 2^31 - 1", who, dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (!empty && (dims[0] > kMaxAxisCells || dims[1] > kMaxAxisCells || dims[2] > kMaxAxisCells)) {
    set_last_error_text("%s: %d x %d x %d cells are more than 2^16 along an axis", who, dims[0], dims[1], dims[2]);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  return SVOSLAM_OK;
}

bool bad_common(const int32_t origin[3], const int32_t dims[3], int32_t r, int32_t E) {
  return !origin || !dims || dims[0] < 0 || dims[1] < 0 || dims[2] < 0 || r < 0 || r > SVOSLAM_MAX_RADIUS_CELLS || E < 0 ||
         E > SVOSLAM_MAX_CORRIDOR_EXTENT;
}

}  // namespace

int field_grow_boxes(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t r, int32_t E, const int32_t *d_seeds,
                     int32_t n, int32_t *d_boxes, int32_t *d_layers, hipStream_t stream) {
  if (bad_common(origin, dims, r, E) || n < 0) return SVOSLAM_ERR_INVALID_ARG;
  long long cells;
  SVO_TRY(region_cells("svoslam_field_grow_boxes", dims, &cells));
  if (n == 0) return SVOSLAM_OK;
  if (!d_seeds || !d_boxes || !d_layers || (cells > 0 && !d_dist2)) return SVOSLAM_ERR_INVALID_ARG;
  const FieldView f = {d_dist2, cells ? dims[0] : 0, cells ? dims[1] : 0, cells ? dims[2] : 0};
  StageScope timed(kStageQuery, stream);
  grow_boxes_kernel<<<cdiv(n, 4), 256, 0, stream>>>(f, origin[0], origin[1], origin[2], r * r, E, d_seeds, n, d_boxes, d_layers);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

int field_path_corridors(const int32_t *d_dist2, const int32_t origin[3], const int32_t dims[3], int32_t r, int32_t E,
                         const int32_t *d_paths, const int32_t *d_lengths, int32_t n_paths, int32_t max_cells, int32_t max_boxes,
                         int32_t *d_boxes, int32_t *d_anchors, int32_t *d_counts, int32_t *d_gaps, hipStream_t stream) {
  if (bad_common(origin, dims, r, E) || n_paths < 0 || max_cells < 0 || max_boxes < 0) return SVOSLAM_ERR_INVALID_ARG;
  long long cells;
  SVO_TRY(region_cells("svoslam_field_path_corridors", dims, &cells));
  if ((long long)n_paths * max_cells > INT_MAX / 3) {
    set_last_error_text("svoslam_field_path_corridors: %d paths of %d cells are more than 2^31 - 1 path entries", n_paths, max_cells);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if ((long long)n_paths * max_boxes > INT_MAX / 6) {
    set_last_error_text("svoslam_field_path_corridors: %d paths of %d boxes are more than 2^31 - 1 box entries", n_paths, max_boxes);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  if (n_paths == 0) return SVOSLAM_OK;
  if (!d_lengths || !d_counts || (cells > 0 && !d_dist2) || (max_cells > 0 && !d_paths) || (max_boxes > 0 && (!d_boxes || !d_anchors)))
    return SVOSLAM_ERR_INVALID_ARG;
  const FieldView f = {d_dist2, cells ? dims[0] : 0, cells ? dims[1] : 0, cells ? dims[2] : 0};
  StageScope timed(kStageQuery, stream);
  path_corridors_kernel<<<cdiv(n_paths, 4), 256, 0, stream>>>(f, origin[0], origin[1], origin[2], r * r, E, d_paths, d_lengths, n_paths,
                                                              max_cells, max_boxes, d_boxes, d_anchors, d_counts, d_gaps);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam

using namespace svoslam;

// abi.hip's idiom; no shared header holds the two, so they are restated here
#define S(stream) reinterpret_cast<hipStream_t>(stream)
#define NEED_DEVICE() SVO_TRY(ensure_device())

extern "C" {

int svoslam_field_grow_boxes(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells,
                             int32_t max_extent, const int32_t *d_seeds, int32_t n, int32_t *d_boxes, int32_t *d_layers, void *stream) {
  NEED_DEVICE();
  return field_grow_boxes(d_dist2, origin_cell, dims, clearance_cells, max_extent, d_seeds, n, d_boxes, d_layers, S(stream));
}

int svoslam_field_path_corridors(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells,
                                 int32_t max_extent, const int32_t *d_paths, const int32_t *d_lengths, int32_t n_paths, int32_t max_cells,
                                 int32_t max_boxes, int32_t *d_boxes, int32_t *d_anchors, int32_t *d_counts, int32_t *d_gaps,
                                 void *stream) {
  NEED_DEVICE();
  return field_path_corridors(d_dist2, origin_cell, dims, clearance_cells, max_extent, d_paths, d_lengths, n_paths, max_cells, max_boxes,
                              d_boxes, d_anchors, d_counts, d_gaps, S(stream));
}

}  // extern "C"
