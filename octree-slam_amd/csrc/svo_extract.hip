// svo_extract.hip -- the map's occupied leaves as a voxel grid (extractVoxelGridFromSVO, svo.cu:498-582, 699-745).
#include "radix_sort.hpp"
#include "svo_build.hpp"
#include "svo_fuse_internal.hpp"
#include "wave_rank.hpp"

namespace svoslam {

// ----------------------------------------------------------------------------
// extraction (svo.cu:498-582, 699-745): level-synchronous BFS with an
// order-preserving compaction per level
// ----------------------------------------------------------------------------
__global__ __launch_bounds__(256) void bfs_count_kernel(const u32 *__restrict__ pool, const u64 *__restrict__ parents,
                                                        int num, unsigned char *__restrict__ mask8,
                                                        u32 *__restrict__ tile_cnt) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  u32 cntv = 0;
  if (i < num) {
    const u64 key = parents[i];
    const int d = (63 - __clzll((long long)key)) / 3;
    bool has_children = true;
    u32 pointer = 0;
    for (int l = d - 1; l >= 0; l--) {  // getOccupiedChildren :515-520
      pointer += (u32)(key >> (3 * l)) & 7u;
      const u32 w0 = pool[2 * (size_t)pointer];
      has_children = (w0 & kFlag) != 0;
      pointer = w0 & kMask;
    }
    u32 m = 0;
    if (has_children) {
      const uint4 *tile = reinterpret_cast<const uint4 *>(pool + 2 * (size_t)pointer);
#pragma unroll
      for (int q = 0; q < 4; q++) {
        const uint4 v = tile[q];
        if ((v.y >> 24) > 127u) m |= 1u << (2 * q);
        if ((v.w >> 24) > 127u) m |= 1u << (2 * q + 1);
      }
    }
    mask8[i] = (unsigned char)m;
    cntv = __popc(m);
  }
  u32 total;
  (void)block256_exclusive_scan(cntv, tmp, total);
  if (threadIdx.x == 0) tile_cnt[blockIdx.x] = total;
}

__global__ __launch_bounds__(256) void bfs_emit_kernel(const u64 *__restrict__ parents, int num,
                                                       const unsigned char *__restrict__ mask8,
                                                       const u32 *__restrict__ tile_prefix, u64 *__restrict__ children) {
  __shared__ u32 tmp[4];
  const int i = blockIdx.x * 256 + threadIdx.x;
  const u32 m = i < num ? mask8[i] : 0u;
  u32 total;
  u32 pos = tile_prefix[blockIdx.x] + block256_exclusive_scan(__popc(m), tmp, total);
  if (i < num) {
    const u64 key = parents[i];
#pragma unroll
    for (int k = 0; k < 8; k++)
      if (m & (1u << k)) children[pos++] = (key << 3) + (u64)k;
  }
}

// voxelGridFromKeys, svo.cu:538-582
__global__ __launch_bounds__(256) void voxel_grid_from_keys_kernel(const u32 *__restrict__ pool, const u64 *__restrict__ keys,
                                                                   int num, float cx, float cy, float cz, float edge,
                                                                   float4 *__restrict__ centers, float4 *__restrict__ colors) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num) return;
  const u64 key = keys[i];
  const int d = (63 - __clzll((long long)key)) / 3;
  u32 node = 0, child = 0;
  for (int l = d - 1; l >= 0; l--) {
    const u32 p = (u32)(key >> (3 * l)) & 7u;
    node = child + p;
    child = pool[2 * (size_t)node] & kMask;
    edge /= 2.0f;
    cx += edge * ((p & 1u) ? 1 : -1);
    cy += edge * ((p & 2u) ? 1 : -1);
    cz += edge * ((p & 4u) ? 1 : -1);
  }
  const u32 val = pool[2 * (size_t)node + 1];
  centers[i] = make_float4(cx, cy, cz, 1.0f);
  colors[i] = make_float4((float)(val & 0xFF) / 255.0f, (float)((val >> 8) & 0xFF) / 255.0f,
                          (float)((val >> 16) & 0xFF) / 255.0f, (float)((val >> 24) & 0xFF) / 255.0f);
}

// The occupied cells at `depth` as BFS keys (leading 1, then one octant triple per level), ascending: a cell is listed iff every
// node on its path has alpha > 127 and every node above it has children.  The keys stay in the workspace (*keys: bfs_a or bfs_b)
// until its next extraction.  Blocking (one 4-byte readback per level).  Shared by the voxel grid and the surface mesh.
int bfs_occupied_keys(svoslam_workspace *ws, const svoslam_pool *pool, int depth, hipStream_t stream, const u64 **keys, int *num_out) {
  *keys = nullptr; *num_out = 0;
  if (pool->pending > 0) SVO_HIP(hipStreamSynchronize(stream));  // (size itself is not needed by the BFS)
  SVO_TRY(ws->reserve_small());  // (zeroed when created: any_valid and the plan's arrival ticket start at zero)
  SVO_TRY(ws->bfs_a.reserve(8));
  const u64 one = 1;
  SVO_HIP(hipMemcpyAsync(ws->bfs_a.ptr, &one, 8, hipMemcpyHostToDevice, stream));
  SVO_HIP(hipStreamSynchronize(stream));
  svoslam::DeviceBuffer *cur = &ws->bfs_a, *nxt = &ws->bfs_b;
  int num = 1;
  for (int lvl = 0; lvl < depth && num > 0; lvl++) {
    const int tiles = (int)cdiv(num, 256);
    SVO_TRY(ws->bfs_mask.reserve((size_t)num));
    SVO_TRY(ws->tile_hist.reserve((size_t)(tiles + 1) * 4));
    bfs_count_kernel<<<tiles, 256, 0, stream>>>(pool->d_data, cur->as<u64>(), num, ws->bfs_mask.as<unsigned char>(), ws->tile_hist.as<u32>());
    row_scan_rows1(ws->tile_hist.as<u32>(), tiles, small_totals(ws), stream);
    unsigned next_num = 0;
    SVO_HIP(hipMemcpyAsync(&next_num, small_totals(ws), 4, hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    if (next_num > 0) {
      SVO_TRY(nxt->reserve((size_t)next_num * 8));
      bfs_emit_kernel<<<tiles, 256, 0, stream>>>(cur->as<u64>(), num, ws->bfs_mask.as<unsigned char>(), ws->tile_hist.as<u32>(), nxt->as<u64>());
      SVO_LAUNCH_CHECK();
    }
    svoslam::DeviceBuffer *t = cur; cur = nxt; nxt = t;
    num = (int)next_num;
  }
  if (num > 0) { *keys = cur->as<u64>(); *num_out = num; }
  return SVOSLAM_OK;
}

int extract_voxel_grid(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const float center[3], float edge,
                       float **d_centers, float **d_colors, int32_t *n_out, hipStream_t stream) {
  if (!ws || !pool || !d_centers || !d_colors || !n_out) return SVOSLAM_ERR_INVALID_ARG;
  if (depth < 1 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_DEPTH;
  *d_centers = nullptr; *d_colors = nullptr; *n_out = 0;
  if (pool->size == 0) return SVOSLAM_OK;
  const u64 *keys = nullptr;
  int num = 0;
  SVO_TRY(bfs_occupied_keys(ws, pool, depth, stream, &keys, &num));
  if (num <= 0) return SVOSLAM_OK;
  float *ce = nullptr, *co = nullptr;
  SVO_HIP(hipMalloc((void **)&ce, (size_t)num * 16));
  SVO_HIP(hipMalloc((void **)&co, (size_t)num * 16));
  voxel_grid_from_keys_kernel<<<cdiv(num, 256), 256, 0, stream>>>(pool->d_data, keys, num, center[0], center[1], center[2], edge,
                                                                  reinterpret_cast<float4 *>(ce), reinterpret_cast<float4 *>(co));
  SVO_LAUNCH_CHECK();
  SVO_HIP(hipStreamSynchronize(stream));
  *d_centers = ce; *d_colors = co; *n_out = num;
  return SVOSLAM_OK;
}

}  // namespace svoslam
