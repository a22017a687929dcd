// svo_surface.hip -- the map's surface as a welded quad mesh, and its PLY writer (own specification, DESIGN.md section 12:
// the reference has nothing like it).
//
// The occupied cells at depth d are those of the voxel extraction (svo_extract.hip: bfs_occupied_keys).  A cell face is part of
// the surface iff the cell behind it lies outside the root cube or is not occupied; faces are ordered by (cell key, direction),
// directions -x +x -y +y -z +z.  The four corners of a face are lattice points of [0, 2^d]^3; one vertex per lattice point in
// use, ordered by the key iz << 2(d+1) | iy << (d+1) | ix, which is what the sort of the 4 x faces corner keys yields.
//
//   surface_mask_kernel   one lane per cell: 6-bit face mask, the cell's colour word, face count per workgroup
//   surface_emit_kernel   one lane per cell: per face its colour and four corner keys
//   radix_sort_pairs      corner keys (3(d+1) bits) with their slot 4 face + corner as the value
//   weld_flag_kernel      run heads of the sorted keys, counted per workgroup
//   weld_scatter_kernel   rank of each run -> quads[slot]; the heads write the vertex positions
#include <stdio.h>
#include <string.h>

#include <vector>

#include "radix_sort.hpp"
#include "stage_timing.hpp"
#include "svo_build.hpp"
#include "svo_fuse_internal.hpp"
#include "wave_rank.hpp"

namespace svoslam {

// is the cell (x, y, z) of the 2^d lattice occupied?  The walk the BFS does for one key: alpha at every level, the children
// flag above the last.  Neighbours share the top of their path with the cell that asks: those loads are cache hits.
__device__ inline bool cell_occupied(const u32 *__restrict__ pool, u32 x, u32 y, u32 z, int d) {
  u32 child = 0;
  for (int l = d - 1; l >= 0; l--) {
    const u32 o = ((x >> l) & 1u) | (((y >> l) & 1u) << 1) | (((z >> l) & 1u) << 2);
    const uint2 w = *reinterpret_cast<const uint2 *>(pool + 2 * (size_t)(child + o));
    if ((w.y >> 24) <= 127u) return false;
    if (l > 0) {
      if (!(w.x & kFlag)) return false;
      child = w.x & kMask;
    }
  }
  return true;
}

// x, y, z of a BFS key (octant bit 0 = x, 1 = y, 2 = z; level 1 most significant)
__device__ inline void cell_coords(u64 key, int d, u32 &x, u32 &y, u32 &z) {
  x = y = z = 0;
  for (int l = 0; l < d; l++) {
    const u32 o = (u32)(key >> (3 * l)) & 7u;
    x |= (o & 1u) << l;
    y |= ((o >> 1) & 1u) << l;
    z |= ((o >> 2) & 1u) << l;
  }
}

__global__ __launch_bounds__(256) void surface_mask_kernel(const u32 *__restrict__ pool, const u64 *__restrict__ keys, int num, int d,
                                                           unsigned char *__restrict__ mask6, u32 *__restrict__ cell_color,
                                                           u32 *__restrict__ tile_cnt, unsigned long long *__restrict__ face_total) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  u32 m = 0;
  if (i < num) {
    const u64 key = keys[i];
    u32 base = 0;  // the cell's own tile: its parent's children
    for (int l = d - 1; l >= 1; l--) base = pool[2 * (size_t)(base + ((u32)(key >> (3 * l)) & 7u))] & kMask;
    const u32 o = (u32)key & 7u;
    u32 sib = 0;  // bit k: sibling k is occupied (the path above is the cell's own, so alpha alone decides)
    const uint4 *tile = reinterpret_cast<const uint4 *>(pool + 2 * (size_t)base);
#pragma unroll
    for (int q = 0; q < 4; q++) {
      const uint4 v = tile[q];
      if ((v.y >> 24) > 127u) sib |= 1u << (2 * q);
      if ((v.w >> 24) > 127u) sib |= 1u << (2 * q + 1);
    }
    cell_color[i] = pool[2 * (size_t)(base + o) + 1];
    u32 x, y, z;
    cell_coords(key, d, x, y, z);
    const u32 N = 1u << d;
#pragma unroll
    for (int dir = 0; dir < 6; dir++) {
      const int axis = dir >> 1;
      const bool up = dir & 1;
      const u32 c = axis == 0 ? x : (axis == 1 ? y : z);
      bool occupied;
      if (((c & 1u) != 0) != up) {  // the neighbour is a sibling
        occupied = (sib >> (o ^ (1u << axis))) & 1u;
      } else if (up ? c + 1 >= N : c == 0) {  // outside the root cube
        occupied = false;
      } else {
        const u32 nc = up ? c + 1 : c - 1;
        occupied = cell_occupied(pool, axis == 0 ? nc : x, axis == 1 ? nc : y, axis == 2 ? nc : z, d);
      }
      if (!occupied) m |= 1u << dir;
    }
    mask6[i] = (unsigned char)m;
  }
  u32 total;
  (void)block256_exclusive_scan(__popc(m), tmp, total);
  if (threadIdx.x == 0) {
    tile_cnt[blockIdx.x] = total;
    atomicAdd(face_total, (unsigned long long)total);  // (the 32-bit scan of tile_cnt wraps beyond 2^32 faces; this does not)
  }
}

// corners of the face `dir`, counter-clockwise seen from outside; a corner is dx | dy << 1 | dz << 2, four of them in 12 bits
#define SVO_FACE(a, b, c, e) ((a) | ((b) << 3) | ((c) << 6) | ((e) << 9))
__device__ inline constexpr u32 face_corners(int dir) {
  return dir == 0 ? SVO_FACE(0u, 4u, 6u, 2u) : dir == 1 ? SVO_FACE(1u, 3u, 7u, 5u) : dir == 2 ? SVO_FACE(0u, 1u, 5u, 4u)
       : dir == 3 ? SVO_FACE(2u, 6u, 7u, 3u) : dir == 4 ? SVO_FACE(0u, 2u, 3u, 1u) : SVO_FACE(4u, 5u, 7u, 6u);
}
#undef SVO_FACE

__global__ __launch_bounds__(256) void surface_emit_kernel(const u64 *__restrict__ keys, int num, int d,
                                                           const unsigned char *__restrict__ mask6, const u32 *__restrict__ cell_color,
                                                           const u32 *__restrict__ tile_prefix, u32 *__restrict__ face_colors,
                                                           u64 *__restrict__ corner_keys) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const u32 m = i < num ? mask6[i] : 0u;
  u32 total;
  u32 f = tile_prefix[blockIdx.x] + block256_exclusive_scan(__popc(m), tmp, total);
  if (i >= num || m == 0) return;
  u32 x, y, z;
  cell_coords(keys[i], d, x, y, z);
  const u32 color = cell_color[i];
  const int s = d + 1;
#pragma unroll
  for (int dir = 0; dir < 6; dir++) {
    if (!(m & (1u << dir))) continue;
    const u32 code = face_corners(dir);
    u64 k[4];
#pragma unroll
    for (int c = 0; c < 4; c++) {
      const u32 b = (code >> (3 * c)) & 7u;
      k[c] = ((u64)(z + ((b >> 2) & 1u)) << (2 * s)) | ((u64)(y + ((b >> 1) & 1u)) << s) | (u64)(x + (b & 1u));
    }
    face_colors[f] = color;
    ulonglong2 *out = reinterpret_cast<ulonglong2 *>(corner_keys + 4 * (size_t)f);
    out[0] = make_ulonglong2(k[0], k[1]);
    out[1] = make_ulonglong2(k[2], k[3]);
    f++;
  }
}

__device__ inline u32 run_head(const u64 *__restrict__ skey, int i, int n) {
  return (i < n && (i == 0 || skey[i] != skey[i - 1])) ? 1u : 0u;
}

__global__ __launch_bounds__(256) void weld_flag_kernel(const u64 *__restrict__ skey, int n, u32 *__restrict__ tile_cnt) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;  // (n <= 2^31 - 1 and the grid is cdiv(n, 256): no overflow)
  u32 total;
  (void)block256_exclusive_scan(run_head(skey, i, n), tmp, total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void weld_scatter_kernel(const u64 *__restrict__ skey, const u32 *__restrict__ slot, int n,
                                                           const u32 *__restrict__ tile_prefix, int d, float cx, float cy, float cz,
                                                           float edge, u32 *__restrict__ quads, float *__restrict__ vertices) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const u32 head = run_head(skey, i, n);
  u32 total;
  const u32 rank = tile_prefix[blockIdx.x] + block256_exclusive_scan(head, tmp, total) + head - 1u;  // runs up to and with mine, less one
  if (i >= n) return;
  quads[slot[i]] = rank;
  if (head) {
    const u64 key = skey[i];
    const int s = d + 1;
    const u64 cm = (1ull << s) - 1ull;
    const int N = 1 << d;
    const float step = edge / (float)N;
    const int ix = (int)(key & cm), iy = (int)((key >> s) & cm), iz = (int)((key >> (2 * s)) & cm);
    float *v = vertices + 3 * (size_t)rank;
    v[0] = cx + (float)(2 * ix - N) * step;
    v[1] = cy + (float)(2 * iy - N) * step;
    v[2] = cz + (float)(2 * iz - N) * step;
  }
}

namespace {
struct SurfaceOut { float *vertices = nullptr; u32 *quads = nullptr, *colors = nullptr; };

int surface_impl(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const float center[3], float edge, SurfaceOut &o,
                 svoslam_surface_stats *stats, hipStream_t stream) {
  const u64 *keys = nullptr;
  int num = 0;
  {
    StageScope bfs(kStageSurfaceBfs, stream);
    SVO_TRY(bfs_occupied_keys(ws, pool, depth, stream, &keys, &num));
  }
  if (num <= 0) return SVOSLAM_OK;
  stats->cells = num;
  // ---- face pass: mask + count, scan, emit (two brackets: the host allocates between them)
  const int tiles = (int)cdiv(num, 256);
  SVO_TRY(ws->bfs_mask.reserve((size_t)num));
  SVO_TRY(ws->surf_color.reserve((size_t)num * 4));
  SVO_TRY(ws->surf_tiles.reserve(16 + (size_t)(tiles + 1) * 4));
  unsigned long long *d_total = ws->surf_tiles.as<unsigned long long>();
  u32 *tile_cnt = ws->surf_tiles.as<u32>() + 4;
  unsigned long long total_faces = 0;
  {
    StageScope faces(kStageSurfaceFaces, stream);
    SVO_HIP(hipMemsetAsync(d_total, 0, 8, stream));
    surface_mask_kernel<<<tiles, 256, 0, stream>>>(pool->d_data, keys, num, depth, ws->bfs_mask.as<unsigned char>(), ws->surf_color.as<u32>(),
                                                   tile_cnt, d_total);
    SVO_LAUNCH_CHECK();
    row_scan_rows1(tile_cnt, tiles, small_totals(ws), stream);
    SVO_LAUNCH_CHECK();
    SVO_HIP(hipMemcpyAsync(&total_faces, d_total, 8, hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
  }
  if (total_faces == 0) return SVOSLAM_OK;
  if (4ull * total_faces > 0x7FFFFFFFull) {
    set_last_error_text("extract_surface_mesh: %llu faces have more than 2^31 - 1 corners (the weld's sort takes an int count)", total_faces);
    return SVOSLAM_ERR_POOL_LIMIT;
  }
  const int nf = (int)total_faces, n = 4 * nf;
  SVO_HIP(hipMalloc((void **)&o.quads, (size_t)nf * 16));
  SVO_HIP(hipMalloc((void **)&o.colors, (size_t)nf * 4));
  const int sort_tiles = radix_sort_num_tiles(n), weld_tiles = (int)cdiv(n, 256);
  SVO_TRY(ws->keys_a.reserve((size_t)n * 8));
  SVO_TRY(ws->keys_b.reserve((size_t)n * 8));
  SVO_TRY(ws->vals_a.reserve((size_t)n * 4));
  SVO_TRY(ws->vals_b.reserve((size_t)n * 4));
  const size_t hist_words = (size_t)256 * sort_tiles > (size_t)weld_tiles ? (size_t)256 * sort_tiles : (size_t)weld_tiles;
  SVO_TRY(ws->tile_hist.reserve((hist_words + 1) * 4));
  {
    StageScope faces(kStageSurfaceFaces, stream);
    surface_emit_kernel<<<tiles, 256, 0, stream>>>(keys, num, depth, ws->bfs_mask.as<unsigned char>(), ws->surf_color.as<u32>(), tile_cnt,
                                                   o.colors, ws->keys_a.as<u64>());
    SVO_LAUNCH_CHECK();
  }
  // ---- weld: sort the corner keys, number the runs, scatter the ranks, write the vertices
  u64 *skey = nullptr;
  u32 *slot = nullptr, n_vert = 0;
  u32 *weld_cnt = ws->tile_hist.as<u32>();  // (free again once the sort has run)
  {
    StageScope weld(kStageSurfaceWeld, stream);
    SVO_TRY(radix_sort_pairs(ws, n, 3 * (depth + 1), stream, &skey, &slot));
    weld_flag_kernel<<<weld_tiles, 256, 0, stream>>>(skey, n, weld_cnt);
    SVO_LAUNCH_CHECK();
    SVO_TRY(exclusive_scan_u32(ws, weld_cnt, (u32)weld_tiles, small_totals(ws), stream));
    SVO_LAUNCH_CHECK();
    SVO_HIP(hipMemcpyAsync(&n_vert, small_totals(ws), 4, hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
  }
  SVO_HIP(hipMalloc((void **)&o.vertices, (size_t)n_vert * 12));
  {
    StageScope weld(kStageSurfaceWeld, stream);
    weld_scatter_kernel<<<weld_tiles, 256, 0, stream>>>(skey, slot, n, weld_cnt, depth, center[0], center[1], center[2], edge, o.quads,
                                                        o.vertices);
    SVO_LAUNCH_CHECK();
  }
  SVO_HIP(hipStreamSynchronize(stream));
  stats->faces = nf;
  stats->vertices = (int32_t)n_vert;
  return SVOSLAM_OK;
}
}  // namespace

int extract_surface_mesh(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const float center[3], float edge,
                         float **d_vertices, uint32_t **d_quads, uint32_t **d_face_colors, svoslam_surface_stats *stats,
                         hipStream_t stream) {
  if (!ws || !pool || !center || !d_vertices || !d_quads || !d_face_colors || !stats) return SVOSLAM_ERR_INVALID_ARG;
  if (depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_DEPTH;
  *d_vertices = nullptr; *d_quads = nullptr; *d_face_colors = nullptr;
  stats->cells = stats->faces = stats->vertices = 0;
  // size == 0 is a pool that was never initialised: pool_init leaves 8 nodes and size only grows, so with fusions pending (size
  // then lags) it is still >= 8 and the stream is drained in bfs_occupied_keys -- as in extract_voxel_grid
  if (pool->size == 0) return SVOSLAM_OK;
  SurfaceOut o;
  const int rc = surface_impl(ws, pool, depth, center, edge, o, stats, stream);
  if (rc != SVOSLAM_OK || stats->faces == 0) {  // nothing stays allocated
    if (rc != SVOSLAM_OK) (void)hipStreamSynchronize(stream);
    if (o.vertices) (void)hipFree(o.vertices);
    if (o.quads) (void)hipFree(o.quads);
    if (o.colors) (void)hipFree(o.colors);
    if (rc != SVOSLAM_OK) stats->cells = stats->faces = stats->vertices = 0;
    return rc;
  }
  *d_vertices = o.vertices; *d_quads = o.quads; *d_face_colors = o.colors;
  return SVOSLAM_OK;
}

// ---- PLY (host only) ---------------------------------------------------------------------------------------------------
static inline void put_u32(std::vector<unsigned char> &b, uint32_t v) {
  b.push_back((unsigned char)v); b.push_back((unsigned char)(v >> 8)); b.push_back((unsigned char)(v >> 16)); b.push_back((unsigned char)(v >> 24));
}

int mesh_write_ply(const char *path, const float *h_vertices, int32_t n_vertices, const uint32_t *h_quads, const uint32_t *h_face_colors,
                   int32_t n_faces, int32_t triangulate) {
  if (!path || n_vertices < 0 || n_faces < 0 || (n_vertices > 0 && !h_vertices) || (n_faces > 0 && (!h_quads || !h_face_colors)))
    return SVOSLAM_ERR_INVALID_ARG;
  for (size_t k = 0; k < 4 * (size_t)n_faces; k++) {
    if (h_quads[k] >= (uint32_t)n_vertices) {
      set_last_error_text("mesh_write_ply: face %zu names vertex %u of %d", k / 4, h_quads[k], n_vertices);
      return SVOSLAM_ERR_INVALID_ARG;
    }
  }
  FILE *fp = fopen(path, "wb");
  if (!fp) {
    set_last_error_text("mesh_write_ply: cannot open '%s' for writing", path);
    return SVOSLAM_ERR_IO;
  }
  bool ok = fprintf(fp,
                    "ply\nformat binary_little_endian 1.0\ncomment libsvoslam_hip surface mesh\nelement vertex %d\nproperty float x\n"
                    "property float y\nproperty float z\nelement face %lld\nproperty list uchar uint vertex_indices\nproperty uchar red\n"
                    "property uchar green\nproperty uchar blue\nproperty uchar alpha\nend_header\n",
                    n_vertices, triangulate ? 2ll * n_faces : (long long)n_faces) > 0;
  std::vector<unsigned char> buf;
  const size_t kFlush = (size_t)1 << 20;
  buf.reserve(kFlush + 64);
  auto flush = [&]() {
    if (ok && !buf.empty()) ok = fwrite(buf.data(), 1, buf.size(), fp) == buf.size();
    buf.clear();
  };
  for (size_t k = 0; ok && k < 3 * (size_t)n_vertices; k++) {
    put_u32(buf, f2bits(h_vertices[k]));
    if (buf.size() >= kFlush) flush();
  }
  auto put_face = [&](int count, uint32_t a, uint32_t b, uint32_t c, uint32_t e, uint32_t color) {
    buf.push_back((unsigned char)count);
    put_u32(buf, a); put_u32(buf, b); put_u32(buf, c);
    if (count == 4) put_u32(buf, e);
    put_u32(buf, color);  // R | G << 8 | B << 16 | A << 24 = the bytes red green blue alpha
  };
  for (size_t f = 0; ok && f < (size_t)n_faces; f++) {
    const uint32_t *q = h_quads + 4 * f;
    if (triangulate) {
      put_face(3, q[0], q[1], q[2], 0, h_face_colors[f]);
      put_face(3, q[0], q[2], q[3], 0, h_face_colors[f]);
    } else {
      put_face(4, q[0], q[1], q[2], q[3], h_face_colors[f]);
    }
    if (buf.size() >= kFlush) flush();
  }
  flush();
  if (fclose(fp) != 0) ok = false;
  if (!ok) {
    (void)remove(path);
    set_last_error_text("mesh_write_ply: writing '%s' failed", path);
    return SVOSLAM_ERR_IO;
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
