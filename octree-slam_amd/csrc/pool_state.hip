// pool_state.hip -- the node pool's host state: its allocation (geometric growth, re-rooting, adopting a re-indexed copy), the size
// bookkeeping of the asynchronous fusion (host size, device-resident size, reservations, the non-blocking readbacks of PoolTracker) and
// checkpoints.  Nothing here knows how a fusion plans or commits: svo_build.hip and svo_keyrange.hip book their reservations and
// readbacks through tracker_* / ensure_device_size / grow_pool; pool_compact.hip and pool_paging.hip move nodes and then say what the
// size is (pool_adopt_storage, pool_set_size).
#include <string.h>

#include <cstdio>
#include <vector>

#include "pool_grid.hpp"
#include "pool_state.hpp"
#include "svo_fuse_internal.hpp"  // average_tile (reroot_kernel)

namespace svoslam {

int tracker_create(svoslam_pool *pool) {
  if (pool->tracker) return SVOSLAM_OK;
  PoolTracker *t = new PoolTracker();
  for (int i = 0; i < PoolTracker::kSlots; i++) t->ev[i] = nullptr;
  bool ok = hipHostMalloc((void **)&t->h_size, PoolTracker::kSlots * 4, hipHostMallocDefault) == hipSuccess;
  for (int i = 0; ok && i < PoolTracker::kSlots; i++) ok = hipEventCreateWithFlags(&t->ev[i], hipEventDisableTiming) == hipSuccess;
  ok = ok && hipMalloc((void **)&t->d_slot, 4) == hipSuccess && memset_sync(t->d_slot, 0, 4) == hipSuccess;
  ok = ok && hipMalloc((void **)&t->d_struct, 4) == hipSuccess && memset_sync(t->d_struct, 0, 4) == hipSuccess;
  pool->tracker = t;
  if (!ok) {  // whatever was created goes away again (events and pinned memory leaked on these paths)
    (void)hipGetLastError();
    pool_tracker_destroy(pool);
    return SVOSLAM_ERR_HIP;
  }
  return SVOSLAM_OK;
}

void pool_tracker_destroy(svoslam_pool *pool) {
  PoolTracker *t = pool ? tracker_of(pool) : nullptr;
  if (!t) return;
  for (int i = 0; i < PoolTracker::kSlots; i++) if (t->ev[i]) (void)hipEventDestroy(t->ev[i]);
  if (t->h_size) (void)hipHostFree(t->h_size);
  if (t->d_slot) (void)hipFree(t->d_slot);
  if (t->d_struct) (void)hipFree(t->d_struct);
  delete t;
  pool->tracker = nullptr;
}

// retire the completed readbacks (wait_all: block until every one has completed)
int tracker_poll(svoslam_pool *pool, bool wait_all) {
  PoolTracker *t = tracker_of(pool);
  if (!t) return SVOSLAM_OK;
  while (t->count > 0) {
    const PoolTracker::InFlight f = t->q[0];
    if (wait_all) SVO_HIP(hipEventSynchronize(t->ev[f.slot]));
    else {
      const hipError_t e = hipEventQuery(t->ev[f.slot]);
      if (e == hipErrorNotReady) { (void)hipGetLastError(); break; }
      SVO_HIP(e);
    }
    pool->size = t->h_size[f.slot];
    pool->pending_bound -= f.bound;
    if (pool->pending_bound < 0) pool->pending_bound = 0;
    if (pool->pending > 0) pool->pending -= 1;
    for (int i = 1; i < t->count; i++) t->q[i - 1] = t->q[i];
    t->count--;
  }
  return SVOSLAM_OK;
}

// before a commit is enqueued: its last kernel stores the new size into h_size[next], which must not be the slot of a
// readback the host has not retired yet (with 8 readbacks in flight the 9th commit overwrote the oldest
// un-polled entry and pool->size jumped ahead and stepped back until the next drain)
int tracker_make_room(svoslam_pool *pool) {
  PoolTracker *t = tracker_of(pool);
  if (!t || t->count < PoolTracker::kSlots) return SVOSLAM_OK;
  SVO_HIP(hipEventSynchronize(t->ev[t->q[0].slot]));  // the oldest readback is long done in practice
  return tracker_poll(pool, false);
}

// after a commit has been enqueued on `stream`
int tracker_push(svoslam_pool *pool, int64_t bound, hipStream_t stream) {
  PoolTracker *t = tracker_of(pool);
  if (!t) return SVOSLAM_OK;
  if (t->count == PoolTracker::kSlots) {  // ring full: the oldest readback is long done in practice
    SVO_HIP(hipEventSynchronize(t->ev[t->q[0].slot]));
    SVO_TRY(tracker_poll(pool, false));
  }
  const int slot = t->next;
  t->next = (t->next + 1) % PoolTracker::kSlots;
  (void)slot;  // h_size[slot] is stored by mip_straddle_kernel (no copy operation between the commit and the next render)
  SVO_HIP(hipEventRecord(t->ev[slot], stream));
  t->q[t->count].slot = slot;
  t->q[t->count].bound = bound;
  t->count++;
  return SVOSLAM_OK;
}

int pool_sync(svoslam_pool *pool, hipStream_t stream) {
  if (!pool) return SVOSLAM_ERR_INVALID_ARG;
  if (tracker_of(pool) && tracker_of(pool)->count > 0) {  // the last commit's readback is the exact size
    SVO_TRY(tracker_poll(pool, true));
  } else if (pool->pending > 0 && pool->d_size) {
    int32_t sz = 0;
    SVO_HIP(hipMemcpyAsync(&sz, pool->d_size, 4, hipMemcpyDeviceToHost, stream));
    SVO_HIP(hipStreamSynchronize(stream));
    pool->size = sz;
  }
  pool->pending = 0;
  // what tracker_poll left of pending_bound is the reservation of plans that have no commit yet: zero unless the
  // structure chain is ahead of its commits
  if (!tracker_of(pool) || tracker_of(pool)->planned_ahead == 0) pool->pending_bound = 0;
  return SVOSLAM_OK;
}

int ensure_device_size(svoslam_pool *pool, hipStream_t stream) {
  if (pool->d_size) return SVOSLAM_OK;
  SVO_HIP(hipMalloc((void **)&pool->d_size, 4));
  SVO_HIP(hipMemcpyAsync(pool->d_size, &pool->size, 4, hipMemcpyHostToDevice, stream));
  SVO_HIP(hipStreamSynchronize(stream));
  return tracker_create(pool);
}

int grow_pool(svoslam_pool *pool, int64_t need_nodes, hipStream_t stream, int64_t live_nodes) {
  if (need_nodes > (int64_t)kMask + 1) return SVOSLAM_ERR_POOL_LIMIT;
  if (need_nodes <= pool->capacity) return SVOSLAM_OK;
  SVO_TRY(pool_sync(pool, stream));  // the copy below needs the exact size
  // live_nodes > size: tiles that plans of the structure chain have written ahead of their commits move along
  const int64_t copy_nodes = live_nodes > pool->size ? (live_nodes < pool->capacity ? live_nodes : pool->capacity) : pool->size;
  int64_t cap = (int64_t)pool->capacity * 2;
  if (cap < need_nodes) cap = need_nodes;
  if (cap > (int64_t)kMask + 1) cap = (int64_t)kMask + 1;
  u32 *fresh = nullptr;
  SVO_HIP(hipMalloc((void **)&fresh, (size_t)cap * 8));
  if (pool->d_data && copy_nodes > 0)
    SVO_HIP(hipMemcpyAsync(fresh, pool->d_data, (size_t)copy_nodes * 8, hipMemcpyDeviceToDevice, stream));
  SVO_HIP(hipStreamSynchronize(stream));
  pool_accel_rebind(pool->d_data, fresh);
  if (pool->d_data) SVO_HIP(hipFree(pool->d_data));
  pool->d_data = fresh;
  pool->capacity = (int32_t)cap;
  return SVOSLAM_OK;
}

// The pool's size is size_nodes from here on: the host knows it exactly, nothing is in flight, no reservation stands, and the device's
// copy (where the pool has one) says the same.  Blocking.  drop_planned: plans of the structure chain whose commit never came (an error
// mid-run) hold no reservation any more -- pool_reset and pool_set_nodes; the other callers leave planned_ahead as it is.
static int pool_publish_size(svoslam_pool *pool, int32_t size_nodes, bool drop_planned) {
  pool->size = size_nodes;
  pool->pending = 0; pool->pending_bound = 0;
  if (drop_planned && tracker_of(pool)) tracker_of(pool)->planned_ahead = 0;
  if (pool->d_size) SVO_HIP(hipMemcpy(pool->d_size, &pool->size, 4, hipMemcpyHostToDevice));
  return SVOSLAM_OK;
}

// a pool that owns nothing: no nodes, no device-resident size (the tracker has its own life: pool_init, pool_tracker_destroy)
void pool_clear_fields(svoslam_pool *pool) {
  pool->d_data = nullptr; pool->size = 0; pool->capacity = 0;
  pool->d_size = nullptr; pool->pending = 0; pool->pending_bound = 0;
}

int pool_init(svoslam_pool *pool, int32_t capacity_nodes, hipStream_t stream) {
  if (!pool) return SVOSLAM_ERR_INVALID_ARG;
  if (capacity_nodes < 8) capacity_nodes = 8;
  pool_clear_fields(pool);
  pool->tracker = nullptr;
  SVO_TRY(grow_pool(pool, capacity_nodes, stream));
  pool_accel_register(pool);
  SVO_HIP(hipMemsetAsync(pool->d_data, 0, 64, stream));  // initOctree, svo.cu:24-31
  pool->size = 8;
  return ensure_device_size(pool, stream);
}

// ---- growing the root ("a correct expandBySize that re-roots the GPU pool") -------------
// The reference's Octree::expandBySize (octree.cpp:362-378) multiplies size_ and, for a GPU-backed root,
// moves nothing (Q16): the old nodes then describe the wrong region.  Re-rooting the linear tree is local:
// the 8 children of the old root (nodes 0..7) move to a fresh tile at the end of the pool, nodes 0..7
// become the children of the NEW root -- all empty except the octant that holds the old root, which gets
// the children flag, the index of that tile and the mean colour its mip pass would give it.  Every other
// node keeps its index, so nothing below has to change.
__global__ void reroot_kernel(u32 *__restrict__ pool, int *__restrict__ d_size, int n0, int octant) {
  __shared__ uint2 old[8];
  uint2 *nodes = reinterpret_cast<uint2 *>(pool);
  if (threadIdx.x < 8) {
    old[threadIdx.x] = nodes[threadIdx.x];
    nodes[n0 + threadIdx.x] = old[threadIdx.x];
  }
  __syncthreads();
  if (threadIdx.x < 8) nodes[threadIdx.x] = make_uint2(0u, 0u);  // initOctree, svo.cu:24-31
  __syncthreads();
  if (threadIdx.x == 0) {
    nodes[octant] = make_uint2(kFlag | ((u32)n0 & kMask), average_tile(pool, (u32)n0));
    if (d_size) *d_size = n0 + 8;
  }
}

// One doubling of the root cube towards `toward` (per axis: the side on which toward lies relative to the
// centre).  center / edge are updated to the new root; the caller fuses with max_depth + 1 from now on to keep
// its resolution.  Blocking.
int pool_expand(svoslam_pool *pool, float center[3], float *edge, const float toward[3], hipStream_t stream) {
  if (!pool || !pool->d_data || !center || !edge || !toward || !(*edge > 0.0f)) return SVOSLAM_ERR_INVALID_ARG;
  SVO_HIP(hipDeviceSynchronize());
  SVO_TRY(pool_sync(pool, stream));
  if ((int64_t)pool->size + 8 > (int64_t)kMask + 1) return SVOSLAM_ERR_POOL_LIMIT;
  SVO_TRY(grow_pool(pool, (int64_t)pool->size + 8, stream));
  // the old root becomes the child on the side AWAY from the growth: octant bit = old centre > new centre
  int octant = 0;
  float nc[3];
  for (int k = 0; k < 3; k++) {
    const bool grow_plus = toward[k] > center[k];
    nc[k] = center[k] + (grow_plus ? *edge : -*edge);
    if (center[k] > nc[k]) octant |= 1 << k;
  }
  reroot_kernel<<<1, 64, 0, stream>>>(pool->d_data, pool->d_size, pool->size, octant);
  SVO_LAUNCH_CHECK();
  pool_accel_invalidate(pool, 0, false);  // every cell of the level grid now lies one level deeper (the words are the same ones)
  SVO_HIP(hipStreamSynchronize(stream));
  pool->size += 8;
  for (int k = 0; k < 3; k++) center[k] = nc[k];
  *edge = *edge * 2.0f;
  return SVOSLAM_OK;
}

// back to initOctree (8 zeroed root children) keeping the allocation.  Blocking.
int pool_reset(svoslam_pool *pool, hipStream_t stream) {
  if (!pool || !pool->d_data) return SVOSLAM_ERR_INVALID_ARG;
  SVO_HIP(hipDeviceSynchronize());
  SVO_TRY(pool_sync(pool, stream));  // drains the size tracker
  SVO_HIP(memset_sync(pool->d_data, 0, 64));
  pool_accel_invalidate(pool, -1);
  return pool_publish_size(pool, 8, true);
}

int pool_reserve(svoslam_pool *pool, int32_t capacity_nodes, hipStream_t stream) {
  if (!pool) return SVOSLAM_ERR_INVALID_ARG;
  return grow_pool(pool, capacity_nodes, stream);
}

// plans of the structure chain whose commit has not been enqueued yet (they hold node indices of the present numbering)
int pool_planned_ahead(svoslam_pool *pool) { return tracker_of(pool) ? tracker_of(pool)->planned_ahead : 0; }

// The pool's nodes now live in `fresh` (size_nodes of them, room for capacity_nodes): the march acceleration data follows
// the pointer as in grow_pool and is invalidated for a full rebuild, the old allocation is freed, host and device size
// and the reservations are reset as in pool_set_nodes.  The caller has synchronised the device and the pool.
int pool_adopt_storage(svoslam_pool *pool, uint32_t *fresh, int32_t size_nodes, int32_t capacity_nodes, hipStream_t stream) {
  SVO_TRY(ensure_device_size(pool, stream));
  tracker_of(pool)->numbering++;  // a svo_fuse_plan without its commit yet is void from here on (commit_impl refuses it)
  pool_accel_rebind(pool->d_data, fresh);
  u32 *old = pool->d_data;
  pool->d_data = fresh;
  pool->capacity = capacity_nodes;
  pool_accel_invalidate(pool, 0, false);  // the same words under new indices
  pool_accel_trim_shadow(pool);           // a deferred-commit shadow sized for a larger capacity goes back too
  if (old) SVO_HIP(hipFree(old));
  return pool_publish_size(pool, size_nodes, false);  // (the caller has refused a pool with plans ahead)
}

// size bookkeeping after nodes were appended behind pool->size by something other than a fusion (pool_paging.hip: graft)
int pool_set_size(svoslam_pool *pool, int32_t size_nodes, hipStream_t stream) {
  SVO_TRY(ensure_device_size(pool, stream));
  return pool_publish_size(pool, size_nodes, false);  // (the caller has refused a pool with plans ahead)
}

// ---- checkpoint / resume -------------------------------------------------------------
// The pool IS the reference's linear tree (the layout OctreeNode::pushToGPU assembles, octree.cpp:41-79:
// 2-word nodes, 0x40000000 children flag, 30-bit child index), so a checkpoint is the node words behind
// a 64-byte header.  The reference's own (de)serialiser is unfinished (addToLinearTree never sets the
// flag, octree.cpp:138-160), so there is no reference byte stream to match.
struct PoolFileHeader {
  char magic[8];        // "SVOPOOL1"
  uint32_t version;     // 1
  int32_t num_nodes;
  float center[3];
  float edge_length;    // half edge of the root cube
  int32_t max_depth;
  uint32_t reserved;
  uint64_t checksum;    // FNV-1a over the node words
  uint8_t pad[16];
};
static_assert(sizeof(PoolFileHeader) == 64, "header is 64 bytes");

static uint64_t fnv1a_words(const u32 *w, size_t n) {
  uint64_t h = 1469598103934665603ull;
  for (size_t i = 0; i < n; i++) h = (h ^ (uint64_t)w[i]) * 1099511628211ull;
  return h;
}

int pool_save(svoslam_pool *pool, const char *path, const float center[3], float edge, int depth, hipStream_t stream) {
  if (!pool || !path || !center || !pool->d_data) return SVOSLAM_ERR_INVALID_ARG;
  SVO_HIP(hipDeviceSynchronize());  // commits may be in flight on other streams
  SVO_TRY(pool_sync(pool, stream));
  const size_t words = 2 * (size_t)pool->size;
  std::vector<u32> host(words);
  SVO_HIP(hipMemcpy(host.data(), pool->d_data, words * 4, hipMemcpyDeviceToHost));
  PoolFileHeader h;
  memset(&h, 0, sizeof(h));
  memcpy(h.magic, "SVOPOOL1", 8);
  h.version = 1; h.num_nodes = pool->size;
  h.center[0] = center[0]; h.center[1] = center[1]; h.center[2] = center[2];
  h.edge_length = edge; h.max_depth = depth;
  h.checksum = fnv1a_words(host.data(), words);
  FILE *f = fopen(path, "wb");
  if (!f) return SVOSLAM_ERR_IO;
  const bool ok = fwrite(&h, sizeof(h), 1, f) == 1 && (words == 0 || fwrite(host.data(), 4, words, f) == words);
  return (fclose(f) == 0 && ok) ? SVOSLAM_OK : SVOSLAM_ERR_IO;
}

// Replaces the pool's contents by num_nodes host nodes (a linear tree in the reference format): validates the child
// pointers, waits for everything in flight, and resets ALL size bookkeeping -- host size, device-resident size,
// reservations of asynchronous fusions.  Blocking.
int pool_set_nodes(svoslam_pool *pool, const uint32_t *h_words, int32_t num_nodes, hipStream_t stream) {
  if (!pool || !h_words || num_nodes < 8 || (num_nodes & 7) != 0) return SVOSLAM_ERR_INVALID_ARG;
  for (size_t i = 0; i < (size_t)num_nodes; i++) {  // every child tile must lie inside the pool
    const u32 w0 = h_words[2 * i];
    if ((w0 & kFlag) && ((w0 & kMask) + 8u > (u32)num_nodes || ((w0 & kMask) & 7u))) return SVOSLAM_ERR_FORMAT;
  }
  SVO_HIP(hipDeviceSynchronize());
  if (!pool->d_data) SVO_TRY(pool_init(pool, num_nodes, stream));
  SVO_TRY(pool_sync(pool, stream));
  SVO_TRY(grow_pool(pool, num_nodes, stream));
  SVO_HIP(hipMemcpy(pool->d_data, h_words, (size_t)num_nodes * 8, hipMemcpyHostToDevice));
  pool_accel_invalidate(pool);
  return pool_publish_size(pool, num_nodes, true);
}

// dst becomes a byte-identical replica of src (same nodes, same size, at least the same capacity).  Blocking: waits
// for the device (either pool may have work in flight on any stream).
int pool_copy(svoslam_pool *dst, svoslam_pool *src, hipStream_t stream) {
  if (!dst || !src || dst == src || !src->d_data) return SVOSLAM_ERR_INVALID_ARG;
  SVO_HIP(hipDeviceSynchronize());
  SVO_TRY(pool_sync(src, stream));
  if (!dst->d_data) SVO_TRY(pool_init(dst, src->capacity, stream));
  SVO_TRY(pool_sync(dst, stream));
  if (dst->capacity < src->capacity) {
    dst->size = 0;  // nothing worth copying over to the larger allocation
    SVO_TRY(grow_pool(dst, src->capacity, stream));
  }
  SVO_HIP(hipMemcpy(dst->d_data, src->d_data, (size_t)src->size * 8, hipMemcpyDeviceToDevice));
  pool_accel_invalidate(dst);
  SVO_HIP(hipDeviceSynchronize());
  SVO_TRY(ensure_device_size(dst, stream));
  return pool_publish_size(dst, src->size, false);
}

int pool_load(svoslam_pool *pool, const char *path, float center[3], float *edge, int *depth, hipStream_t stream) {
  if (!pool || !path) return SVOSLAM_ERR_INVALID_ARG;
  FILE *f = fopen(path, "rb");
  if (!f) return SVOSLAM_ERR_IO;
  PoolFileHeader h;
  if (fread(&h, sizeof(h), 1, f) != 1 || memcmp(h.magic, "SVOPOOL1", 8) != 0 || h.version != 1 || h.num_nodes < 8 ||
      (h.num_nodes & 7) != 0) {
    fclose(f);
    return SVOSLAM_ERR_FORMAT;
  }
  const size_t words = 2 * (size_t)h.num_nodes;
  std::vector<u32> host(words);
  const bool ok = fread(host.data(), 4, words, f) == words;
  fclose(f);
  if (!ok || fnv1a_words(host.data(), words) != h.checksum) return SVOSLAM_ERR_FORMAT;
  SVO_TRY(pool_set_nodes(pool, host.data(), h.num_nodes, stream));
  if (center) { center[0] = h.center[0]; center[1] = h.center[1]; center[2] = h.center[2]; }
  if (edge) *edge = h.edge_length;
  if (depth) *depth = h.max_depth;
  return SVOSLAM_OK;
}

__global__ void pool_structure_begin_kernel(int *__restrict__ d_struct, const int *__restrict__ d_size) {
  if (threadIdx.x == 0 && blockIdx.x == 0) *d_struct = *d_size;
}

// The structure chain (for callers that do not render every frame: one rank of a frame-sharded session).  A plan reads
// only the pool's STRUCTURE words (children flags and links), and those are final once the splits of the previous frame
// are in -- its leaf blend and mip levels write colour words only.  svo_fuse_plan_structure = plan + split_all (links
// included) in one go, numbering its tiles from a size that follows the PLANS (d_struct); it needs no commit to have
// finished, only the previous svo_fuse_plan_structure (same stream, or ordered by the caller).  The commits -- leaf kernel +
// straddlers, as after svo_fuse_split_early -- follow in order on another stream.  Frames then cost the longer of the two
// chains instead of their sum.  The caller keeps a ray march of frame k away from the structure of frame k+1: no
// svo_fuse_plan_structure(k+1) before the march of frame k is done.  pool_structure_begin: once, after everything
// earlier on the pool has completed in stream order (d_struct := the pool's size).
int pool_structure_begin(svoslam_pool *pool, hipStream_t stream) {
  if (!pool) return SVOSLAM_ERR_INVALID_ARG;
  if (pool->size == 0) SVO_TRY(pool_init(pool, 8, stream));
  SVO_TRY(ensure_device_size(pool, stream));
  pool_structure_begin_kernel<<<1, 64, 0, stream>>>(tracker_of(pool)->d_struct, pool->d_size);
  SVO_LAUNCH_CHECK();
  return SVOSLAM_OK;
}

}  // namespace svoslam
