// pool_state.hpp -- the node pool's host state: allocation, size bookkeeping of the asynchronous fusion, checkpoints (pool_state.hip).
// The pool_* functions are for every translation unit.  PoolTracker and the tracker_* / ensure_device_size / grow_pool functions are
// internal: for the units that enqueue commits or move the pool's nodes (svo_build.hip, svo_keyrange.hip, pool_compact.hip,
// pool_paging.hip).
#pragma once
#include "common.hpp"

namespace svoslam {
int pool_init(svoslam_pool *pool, int32_t capacity_nodes, hipStream_t stream);
void pool_clear_fields(svoslam_pool *pool);  // the fields of a pool that owns nothing (what it owned has been freed, or never existed)
int pool_reserve(svoslam_pool *pool, int32_t capacity_nodes, hipStream_t stream);
int pool_sync(svoslam_pool *pool, hipStream_t stream);
int pool_reset(svoslam_pool *pool, hipStream_t stream);
int pool_expand(svoslam_pool *pool, float center[3], float *edge, const float toward[3], hipStream_t stream);
void pool_tracker_destroy(svoslam_pool *pool);
int pool_save(svoslam_pool *pool, const char *path, const float center[3], float edge, int depth, hipStream_t stream);
int pool_load(svoslam_pool *pool, const char *path, float center[3], float *edge, int *depth, hipStream_t stream);
int pool_set_nodes(svoslam_pool *pool, const uint32_t *h_words, int32_t num_nodes, hipStream_t stream);
int pool_copy(svoslam_pool *dst, svoslam_pool *src, hipStream_t stream);
int pool_planned_ahead(svoslam_pool *pool);
int pool_adopt_storage(svoslam_pool *pool, uint32_t *fresh, int32_t size_nodes, int32_t capacity_nodes, hipStream_t stream);
int pool_set_size(svoslam_pool *pool, int32_t size_nodes, hipStream_t stream);
int pool_structure_begin(svoslam_pool *pool, hipStream_t stream);

// ---- non-blocking size tracking of the asynchronous fusion ----------------------------------------
// Every commit copies the new size (4 bytes) to a pinned host slot behind an event.  The next plan polls
// the events: each completed one makes pool->size current up to that commit and releases its worst-case
// reservation, so the host learns the true size a frame or two late WITHOUT ever waiting for the device.
struct PoolTracker {
  static constexpr int kSlots = 8;  // == the modulus in mip_straddle_kernel
  int32_t *h_size = nullptr;  // pinned, device-visible [kSlots]: the commit's last kernel stores the new size itself
  int *d_slot = nullptr;      // device: slot the next commit writes (advances with `next` below, once per commit)
  int *d_struct = nullptr;    // device: the pool's size as the STRUCTURE chain sees it (svo_fuse_plan_structure; set from d_size by pool_structure_begin)
  hipEvent_t ev[kSlots];
  struct InFlight { int slot; int64_t bound; };
  InFlight q[kSlots];  // oldest first
  int count = 0, next = 0;
  int planned_ahead = 0;  // svo_fuse_plan_structure calls whose commit has not been enqueued yet (their reservations must survive pool_sync)
  uint32_t numbering = 0;  // bumped when every node index changes (pool_adopt_storage): a plan holds indices of the numbering it read
};

inline PoolTracker *tracker_of(svoslam_pool *pool) { return reinterpret_cast<PoolTracker *>(pool->tracker); }
int tracker_create(svoslam_pool *pool);
int tracker_poll(svoslam_pool *pool, bool wait_all);                        // retire the completed readbacks (wait_all: block until every one has completed)
int tracker_make_room(svoslam_pool *pool);                                  // before a commit is enqueued
int tracker_push(svoslam_pool *pool, int64_t bound, hipStream_t stream);    // after a commit has been enqueued on `stream`
int ensure_device_size(svoslam_pool *pool, hipStream_t stream);
int grow_pool(svoslam_pool *pool, int64_t need_nodes, hipStream_t stream, int64_t live_nodes = 0);
}  // namespace svoslam
