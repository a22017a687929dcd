// pool_compact.hip -- compacting re-index of a pool: the tiles reachable from the root tile, in canonical order.
//
// svoslam_pool_evict_subtree (pool_paging.hip) pages a sub-tree out and zeroes its tiles, but node indices are never
// re-used, so the allocation keeps its size.  This is the operation that hands the memory back: every reachable tile moves
// to a fresh allocation, breadth-first from tile 0 -- each level in the order of the parent nodes' NEW indices, then octant
// 0..7: the order evict uses below a node, applied from the root (the project's own specification; the reference has no
// counterpart) -- and word0 of every node with children is re-pointed at the new place of its child tile.  The order is
// canonical: two pools that hold the same tree hold the same bytes afterwards.
//
// Level-synchronous, on the device except for ONE 8-byte readback per level (the size of the next frontier and, beside it, the
// malformed-index flag, so that a bad index ends the call at the level after the one that met it):
//   count   flagged children per tile of the frontier
//   scan    exclusive_scan_u32 (radix_sort.hip)
//   emit    the level's tiles to their FINAL place in the new pool (sequential writes: the level's tiles are new tiles
//           level_base .. level_base + n), word0 re-pointed, and the children's old tile indices to the next frontier
// The frontiers are one array: level k's frontier starts at entry level_base(k), so their concatenation IS the old-tile map
// the caller may ask for (d_old_tile), and no buffer is allocated per level: the map and the counts, sized once from
// size_before / 8.
//
// Thread mapping: 8 lanes per tile, one uint2 (= one node) per lane, so a wavefront moves 8 whole tiles with coalesced
// 8-byte accesses (page_count_kernel / page_emit_kernel give each lane a 64-byte line of its own: eight 8-byte loads per
// lane, 64 lines in flight per wavefront instruction).  A node's rank among the flagged children of its tile is a popcount
// of the wavefront's ballot masked to the lane's group of 8: no LDS.
//
// Malformed (foreign) pools end the call, they never spin a kernel: a child index that is not a multiple of 8 or lies outside
// size_before is replaced by tile 0 in the frontier (so that no launch reads out of bounds) and flagged, and the host checks
// before every emit launch that the tiles visited so far plus the next frontier fit size_before / 8 -- a cycle or a shared
// tile exceeds that after at most size_before / 8 tiles.  The pool is untouched on every error: the walk only reads it.
#include <algorithm>

#include "pool_grid.hpp"
#include "pool_state.hpp"
#include "radix_sort.hpp"
#include "svo_build.hpp"

namespace svoslam {

typedef uint32_t u32;

constexpr int kCompactThreads = 256;  // 32 tiles per workgroup

// flagged children of the lane's tile (bits 0..7 = octants), from the ballot of the whole wavefront
__device__ __forceinline__ u32 tile_child_mask(bool flagged) {
  const unsigned long long b = __ballot(flagged);
  return (u32)(b >> (threadIdx.x & 56u)) & 0xffu;  // (workgroups are whole wavefronts: lane = threadIdx.x & 63)
}

__device__ __forceinline__ bool child_index_ok(u32 child, u32 size_before) {
  return (child & 7u) == 0u && child <= size_before - 8u;  // size_before >= 8
}

__global__ __launch_bounds__(kCompactThreads) void compact_count_kernel(const uint2 *__restrict__ old_nodes, const u32 *__restrict__ tiles, u32 n,
                                                                        u32 *__restrict__ count) {
  const u32 t = blockIdx.x * (u32)kCompactThreads + threadIdx.x;
  const u32 tile = t >> 3, j = t & 7u;
  const bool live = tile < n;
  u32 w0 = 0;
  if (live) w0 = old_nodes[(size_t)tiles[tile] + j].x;
  const u32 mask = tile_child_mask(live && (w0 & kFlag));
  if (live && j == 0) count[tile] = (u32)__popc(mask);
}

// tile `i` of the frontier becomes new tile level_base + i; its flagged children become new tiles next_base + offset[i] + rank
__global__ __launch_bounds__(kCompactThreads) void compact_emit_kernel(const uint2 *__restrict__ old_nodes, const u32 *__restrict__ tiles, u32 n,
                                                                       const u32 *__restrict__ offset, u32 level_base, u32 next_base, u32 size_before,
                                                                       uint2 *__restrict__ new_nodes, u32 *__restrict__ next_tiles,
                                                                       u32 *__restrict__ bad) {
  const u32 t = blockIdx.x * (u32)kCompactThreads + threadIdx.x;
  const u32 tile = t >> 3, j = t & 7u;
  const bool live = tile < n;
  uint2 nd = make_uint2(0u, 0u);
  if (live) nd = old_nodes[(size_t)tiles[tile] + j];
  const bool flagged = live && (nd.x & kFlag);
  const u32 mask = tile_child_mask(flagged);
  if (flagged) {
    const u32 k = offset[tile] + (u32)__popc(mask & ((1u << j) - 1u));
    u32 child = nd.x & kMask;
    if (!child_index_ok(child, size_before)) { child = 0u; atomicOr(bad, 1u); }
    next_tiles[k] = child;
    nd.x = kFlag | (((next_base + k) * 8u) & kMask);
  }
  if (live) new_nodes[(size_t)(level_base + tile) * 8u + j] = nd;
}

int pool_compact(svoslam_pool *pool, int32_t capacity_nodes, uint32_t *d_old_tile, svoslam_compact_stats *stats, hipStream_t stream) {
  if (!pool || !pool->d_data) return SVOSLAM_ERR_INVALID_ARG;
  SVO_HIP(hipDeviceSynchronize());
  SVO_TRY(pool_sync(pool, stream));
  if (pool_planned_ahead(pool) > 0 || pool_shadow_pending(pool)) return SVOSLAM_ERR_INVALID_ARG;
  const int32_t size_before = pool->size, capacity_before = pool->capacity;
  if (size_before < 8) return SVOSLAM_ERR_INVALID_ARG;
  const u32 tile_cap = (u32)size_before / 8u;  // no tree visits more tiles than the pool holds
  // the new allocation: its final size when that is known now, else room for size_before nodes (trimmed below)
  const int64_t alloc_nodes = capacity_nodes <= 0 ? (int64_t)capacity_before : std::max<int64_t>(capacity_nodes, size_before);
  if (alloc_nodes > (int64_t)kMask + 1) return SVOSLAM_ERR_POOL_LIMIT;

  svoslam_workspace ws;
  DeviceBuffer map, count, small;
  u32 *fresh = nullptr;
  auto cleanup = [&]() { map.release(); count.release(); small.release(); ws.release_all(); };
  auto fail = [&](int rc) { cleanup(); if (fresh) (void)hipFree(fresh); return rc; };
  int rc = SVOSLAM_OK;
  if (!d_old_tile && (rc = map.reserve((size_t)tile_cap * 4)) != SVOSLAM_OK) return fail(rc);
  if ((rc = count.reserve((size_t)tile_cap * 4)) != SVOSLAM_OK) return fail(rc);
  if ((rc = small.reserve(8)) != SVOSLAM_OK) return fail(rc);
  if ((rc = ws.scan_tmp.reserve(((size_t)tile_cap / 256 + 1) * 4)) != SVOSLAM_OK) return fail(rc);  // the scan's chunk sums (chunks hold >= 256 entries): no growth inside the walk
  u32 *d_map = d_old_tile ? d_old_tile : map.as<u32>();
  u32 *d_total = small.as<u32>(), *d_bad = small.as<u32>() + 1;
  if (hipMalloc((void **)&fresh, (size_t)alloc_nodes * 8) != hipSuccess) { (void)hipGetLastError(); fresh = nullptr; return fail(SVOSLAM_ERR_OOM); }
  if (hipMemsetAsync(small.ptr, 0, 8, stream) != hipSuccess || hipMemsetAsync(d_map, 0, 4, stream) != hipSuccess) return fail(SVOSLAM_ERR_HIP);  // frontier of level 0 = tile 0

  const uint2 *old_nodes = reinterpret_cast<const uint2 *>(pool->d_data);
  u32 level_base = 0, n = 1;
  int levels = 0;
  while (n > 0) {
    const unsigned blocks = cdiv((long long)n * 8, kCompactThreads);
    compact_count_kernel<<<blocks, kCompactThreads, 0, stream>>>(old_nodes, d_map + level_base, n, count.as<u32>());
    if ((rc = exclusive_scan_u32(&ws, count.as<u32>(), n, d_total, stream)) != SVOSLAM_OK) return fail(rc);
    u32 back[2] = {0u, 0u};  // {next frontier's size, bad index seen by an earlier level's emit}: `small` holds them side by side
    if (hipMemcpyAsync(back, d_total, 8, hipMemcpyDeviceToHost, stream) != hipSuccess || hipStreamSynchronize(stream) != hipSuccess) return fail(SVOSLAM_ERR_HIP);
    if (back[1]) return fail(SVOSLAM_ERR_FORMAT);
    const u32 next_n = back[0], next_base = level_base + n;
    if ((uint64_t)next_base + next_n > (uint64_t)tile_cap) return fail(SVOSLAM_ERR_FORMAT);  // a cycle or a shared tile: before anything is written past the buffers
    compact_emit_kernel<<<blocks, kCompactThreads, 0, stream>>>(old_nodes, d_map + level_base, n, count.as<u32>(), level_base, next_base, (u32)size_before,
                                                                 reinterpret_cast<uint2 *>(fresh), d_map + next_base, d_bad);
    levels++;
    level_base = next_base;
    n = next_n;
  }
  // The per-level readback sees what the emits BEFORE it flagged, so this one covers the emits nothing was read after; it is
  // also the wait for the last emit (and its launch status) before the pool takes the new allocation over.
  u32 bad = 0;
  if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&bad, d_bad, 4, hipMemcpyDeviceToHost, stream) != hipSuccess ||
      hipStreamSynchronize(stream) != hipSuccess) return fail(SVOSLAM_ERR_HIP);
  if (bad) return fail(SVOSLAM_ERR_FORMAT);
  const int32_t size_after = (int32_t)(level_base * 8u);
  int32_t capacity_after = (int32_t)alloc_nodes;
  if (capacity_nodes > 0 && std::max(capacity_nodes, size_after) < capacity_after) {  // trim: the size was not known before the walk
    capacity_after = std::max(capacity_nodes, size_after);
    u32 *trimmed = nullptr;
    if (hipMalloc((void **)&trimmed, (size_t)capacity_after * 8) != hipSuccess) { (void)hipGetLastError(); return fail(SVOSLAM_ERR_OOM); }
    if (hipMemcpy(trimmed, fresh, (size_t)size_after * 8, hipMemcpyDeviceToDevice) != hipSuccess) { (void)hipFree(trimmed); return fail(SVOSLAM_ERR_HIP); }
    if (hipDeviceSynchronize() != hipSuccess) { (void)hipFree(trimmed); return fail(SVOSLAM_ERR_HIP); }
    (void)hipFree(fresh);
    fresh = trimmed;
  }
  cleanup();
  if ((rc = pool_adopt_storage(pool, fresh, size_after, capacity_after, stream)) != SVOSLAM_OK) {
    if (pool->d_data != fresh) (void)hipFree(fresh);  // refused before the pool took it over
    return rc;
  }
  if (stats) {
    stats->size_before = size_before; stats->size_after = size_after;
    stats->capacity_before = capacity_before; stats->capacity_after = capacity_after;
    stats->levels = levels; stats->tiles_dropped = (size_before - size_after) / 8;
  }
  return SVOSLAM_OK;
}

}  // namespace svoslam
