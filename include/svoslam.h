/*
 * svoslam.h -- C ABI of libsvoslam_hip.so, the MI355X (gfx950) drop-in for the
 * GPU kernel API of dkotfis/Octree-SLAM (the "L3" free functions of
 * SURVEY.md section 8b).  Plain pointers and sizes only; no C++/torch types.
 *
 * Conventions
 *  - every pointer named d_* is DEVICE memory (HBM); h_* is host memory;
 *  - `stream` is a hipStream_t passed as void* (NULL = the default stream);
 *    calls enqueue work on it and return without synchronising unless the
 *    comment says "blocking" (the reference API is blocking everywhere);
 *  - vectors are packed floats: vec3 = 3 floats (12 B, glm::vec3 layout),
 *    vec4 = 4 floats; mat4 = 16 floats column-major (glm::mat4 layout);
 *  - every function returns SVOSLAM_OK (0) or a negative svoslam_status; the
 *    reference returns void and checks nothing (SURVEY.md 8b "Errors");
 *  - the library fails loudly (SVOSLAM_ERR_NO_DEVICE) when no gfx950 device is
 *    present: there is no CPU fallback.
 *
 * Each entry point cites the reference declaration it replaces
 * (paths relative to the reference checkout).
 */
#ifndef SVOSLAM_H_
#define SVOSLAM_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVOSLAM_ABI_VERSION 1

typedef enum {
  SVOSLAM_OK = 0,
  SVOSLAM_ERR_INVALID_ARG = -1,
  SVOSLAM_ERR_NO_DEVICE = -2,
  SVOSLAM_ERR_HIP = -3,
  SVOSLAM_ERR_OOM = -4,
  SVOSLAM_ERR_DEPTH = -5,      /* max_depth outside [1, SVOSLAM_MAX_DEPTH] */
  SVOSLAM_ERR_POOL_LIMIT = -6, /* pool would exceed 2^30 nodes (30-bit child index); svoslam_extract_surface_mesh: the surface has
                                  more than (2^31 - 1) / 4 faces (its 4 x faces corner keys are sorted with an int count) */
  SVOSLAM_ERR_TRACKING_LOST = -7,
  SVOSLAM_ERR_IO = -8,         /* file could not be opened / read / written */
  SVOSLAM_ERR_FORMAT = -9      /* file is not what it should be (magic, size, checksum, structure) */
} svoslam_status;

#define SVOSLAM_MAX_DEPTH 16
#define SVOSLAM_FLAG_CHILDREN 0x40000000u /* word0 bit 30, svo.cu:130 */
#define SVOSLAM_CHILD_MASK 0x3FFFFFFFu    /* word0 bits 0-29, svo.cu:136 */

int svoslam_abi_version(void);
const char *svoslam_status_string(int status);

/* Library-wide settings (SURVEY section 5 "config / flags": the reference has compile-time constants and one #define,
 * include/octree_slam/world/svo/svo.h:8).  One struct through the ABI; a process may also preset it with the environment
 * variable SVOSLAM_CONFIG = "name=value,name=value" (field names below; tools and child-process tests), read once when the
 * library first needs a setting.  svoslam_config_set takes effect for objects created afterwards (cameras, runners) and for
 * the next render / fusion call.  -1 = automatic where noted. */
typedef struct svoslam_config {
  int32_t march_bricks;     /* 1: reference-mode renders of this library's pools march over occupancy bricks (0: the tree march) */
  int32_t track_mode;       /* 0: automatic (one launch per frame; its streaming form for large images); 1: the launch chain (two
                               launches per ICP iteration: several PROCESSES sharing one device); 2: the register-resident one-launch
                               form forced whatever the image size (tests) */
  int32_t track_workers;    /* 0: automatic; > 0: cap on the worker workgroups of the one-launch tracker */
  int32_t track_stream;     /* 1: large images use the streaming one-launch form; 0: coarsest level in one launch, then the chain */
  int32_t runner_deferred;  /* frame scheduler: deferred commits -1 automatic (on up to 640x480-class images), 0, 1 */
  int32_t runner_lead;      /* commits the host may run ahead of the device: -1 automatic */
  int32_t runner_prio;      /* stream priorities (map stream highest): -1 automatic, 0, 1 */
  int32_t runner_replicas;  /* retired; must be 1 (two map replicas marched alternately were measured slower: DESIGN.md) */
  int32_t runner_timeline;  /* 1: HIP-event marks at the stage boundaries (svoslam_runner_timeline); costs ~6 % */
  int32_t sort_pairs;       /* 1: force the (key, index) pair sort instead of the packed one-word sort */
  int32_t graphs;           /* retired; must be 0 (launch sequences replayed as graphs were measured slower: DESIGN.md) */
  int32_t march_ahead;      /* brick march: n >= 0 (default 60): past its first n steps a ray is marched in BURSTS of three samples -- the
                               current one and two reached by advancing with the previous step's level, their entries requested
                               together -- and follows the burst as long as each step ends on that level (results identical; overlaps
                               the round trips of a render's long rays); -1: one sample per iteration throughout */
  int32_t reserved[4];
} svoslam_config;
int svoslam_config_get(svoslam_config *out);
int svoslam_config_set(const svoslam_config *in);
/* last HIP error text seen by the calling thread (empty string if none) */
const char *svoslam_last_error(void);
/* name of the device the library runs on, e.g. "gfx950:..."; NULL if none */
const char *svoslam_device_arch(void);

/* ------------------------------------------------------------------------
 * Node pool.  Same layout as the reference (common_types.h:75-79, svo.cu):
 * node i = words 2i, 2i+1; word0 = children flag | 30-bit index of the first
 * of 8 contiguous children; word1 = R | G<<8 | B<<16 | A<<24; nodes 0-7 are
 * the root's children.  Unlike the reference (realloc + whole-pool copy per
 * frame, svo.cu:663-668) the pool keeps spare capacity and grows geometrically.
 * ---------------------------------------------------------------------- */
typedef struct {
  uint32_t *d_data;    /* 2*capacity words, device */
  int32_t size;        /* nodes in use (the reference's octree_size); exact unless `pending` > 0 */
  int32_t capacity;    /* nodes allocated */
  int32_t *d_size;     /* device-resident copy of the size (kept by the library; NULL for foreign pools) */
  int32_t pending;     /* asynchronous fusion calls enqueued since `size` was last exact */
  int64_t pending_bound; /* upper bound on the nodes those calls can add */
  void *tracker;       /* library-internal: non-blocking size readbacks of the asynchronous calls (NULL until first use) */
} svoslam_pool;

/* replaces svo::initOctree (svo.cu:24-31): 8 zeroed root children */
int svoslam_pool_init(svoslam_pool *pool, int32_t capacity_nodes, void *stream);
int svoslam_pool_reserve(svoslam_pool *pool, int32_t capacity_nodes, void *stream);
int svoslam_pool_free(svoslam_pool *pool);
/* back to the 8 zeroed root children of initOctree; the allocation is kept.  Blocking: waits for the whole device. */
int svoslam_pool_reset(svoslam_pool *pool, void *stream);
/* makes pool->size exact again after asynchronous fusion calls (one stream sync + 4-byte readback) */
int svoslam_pool_sync(svoslam_pool *pool, void *stream);
/* Growing the mapped volume (a correct Octree::expandBySize, octree.cpp:362-378 -- the reference
 * rescales size_ without moving a node, Q16).  One doubling of the root cube towards `toward`: the old
 * root's children move to a new tile, nodes 0..7 become the new root's children, the one holding the old
 * root is flagged and coloured with its mean; all other node indices are unchanged.  center[3] and
 * *edge_length (half edge) are updated; fuse with max_depth + 1 afterwards to keep the resolution.  Blocking. */
int svoslam_pool_expand(svoslam_pool *pool, float center[3], float *edge_length, const float toward[3], void *stream);
/* Checkpoint / resume of a map.  The file is the linear tree as it sits in HBM -- the
 * layout OctreeNode::pushToGPU assembles (src/world/octree.cpp:41-79) -- behind a 64-byte header
 * (magic "SVOPOOL1", node count, root centre / half edge / depth, FNV-1a checksum).  Blocking; both wait
 * for the whole device first.  load() verifies the checksum and that every child tile lies inside the
 * pool, (re)allocates the pool and returns the root parameters (each may be NULL). */
int svoslam_pool_save(svoslam_pool *pool, const char *path, const float center[3], float edge_length, int32_t max_depth,
                      void *stream);
/* Tells the library that the pool's node memory was written behind its back (e.g. a hipMemcpy into pool->d_data):
 * derived data it keeps per pool -- the level grid of the ray march -- is rebuilt at the next render.  Pools must
 * otherwise be modified through the library only.  Host state only, no device access. */
int svoslam_pool_touch(svoslam_pool *pool);
/* What the ray march of this pool currently runs on (host state only; round 5: the fallback to the tree march when the 16 GiB
 * occupancy-brick field does not fit beside other pools / ranks of the device used to be silent): *has_grid = the level-8 grid
 * exists, *brick_state = 1 bricks in use, 0 not built (no reference-mode render yet, svoslam_config.march_bricks = 0, or a pool
 * deeper than any shape), -1 the field could not be allocated -- the pool is marched through the tree (correct, slower);
 * *brick_shift = the shape (0: depth <= 12, 1: depth 13 / 14, -1: none).  Any of the pointers may be NULL. */
int svoslam_pool_march_accel(const svoslam_pool *pool, int32_t *has_grid, int32_t *brick_state, int32_t *brick_shift);
/* A read-only view of the tables the march of this pool reads, and of their upkeep state (tests and diagnostics: DESIGN.md
 * section 4, tests/accel_ref.py states the rules the tables follow).  Host state and device ADDRESSES only: nothing is launched,
 * refreshed, allocated or invalidated, so looking does not change what is looked at; the caller synchronises the device before
 * it reads through the addresses.  A pool that is not registered gives all zeros. */
typedef struct svoslam_accel_view {
  void *grid;          /* uint2[2^24] level-8 grid, the pyramid of levels 1..7 behind it at entry 2^24; NULL before the first render */
  void *bricks;        /* uint16 brick field (16 GiB, addressed by window cell); NULL: none */
  void *brick_touched; /* uint32[8192]: one bit per 64 KB group of the field that holds anything */
  void *dirty[2];      /* the two dirty states (uint32 words, laid out as the offsets below say); NULL before the first commit / render */
  int32_t valid, bricks_valid, brick_shift, mip_consistent, max_depth, deferred_pending;  /* as the host sees them */
  int32_t bricks_failed;
  uint32_t epoch;            /* of the latest deferred commit: while one is pending it marks dirty[epoch & 1] */
  uint32_t node0_served;     /* refreshes so far; the latest wrote node 0's word to dirty[0][node0_offset + ((node0_served - 1) & 1)] */
  uint32_t brick_served[2];  /* per state: refreshes that served its rings; the latest wrote mark [(brick_served - 1) & 1] */
  /* word offsets into a dirty state: bitmap of the level-5 blocks [dirty_words], list of marked blocks, its count, node 0's two
   * words, the stale-brick ring (count, two marks behind it, entries [brick_list_cap]), one bit per brick "in this ring"
   * [brick_bits_words], the sibling ring (count, two marks, entries [sib_list_cap]) */
  int32_t dirty_words, list_offset, count_offset, node0_offset, brick_count_offset, brick_list_offset, brick_list_cap,
      brick_bits_offset, brick_bits_words, sib_count_offset, sib_list_offset, sib_list_cap, state_words;
} svoslam_accel_view;
int svoslam_pool_accel_view(const svoslam_pool *pool, svoslam_accel_view *view);
/* Replaces the pool's contents by num_nodes host nodes (2 words each, reference format; child pointers validated) and
 * resets all size bookkeeping incl. the device-resident size the asynchronous fusion allocates from.  Blocking. */
int svoslam_pool_set_nodes(svoslam_pool *pool, const uint32_t *h_words, int32_t num_nodes, void *stream);
/* Out-of-core paging of sub-trees through the linear-tree format (the reference's unfinished
 * OctreeNode::pushToGPU / pullToCPU / addToLinearTree / pullFromLinearTree, src/world/octree.cpp:41-169).
 * evict: the sub-tree below the node reached by `path` (octants 0..7 from the root, `levels` of them; the node must have
 *   children) is written to `file` as a stand-alone linear tree (2-word nodes, bit 30 = children, low 30 bits = index
 *   of the first child inside the file's own array, the sub-tree's 8 top nodes first) plus the original tile indices;
 *   in the pool the node becomes childless (it keeps its colour word) and the tiles are zeroed.
 * restore: the tiles return to the indices they came from; the pool is then bit-identical to one that was never
 *   paged, also when other parts of the map were fused meanwhile (resume == uninterrupted).  Refused with
 *   SVOSLAM_ERR_INVALID_ARG when the cube has been fused into while it was out.
 * svoslam_subtree_file_nodes: the file's linear tree as host words (free() them) -- a pool of its own for
 *   svoslam_pool_set_nodes.  Node indices are never re-used, so eviction alone does not shrink the allocation:
 *   svoslam_pool_compact (below) hands the memory back, and svoslam_pool_graft_subtree brings a paged-out cube back
 *   into a pool whose nodes have been renumbered since.  Blocking.
 * restore after a compaction: the tile indices in the file then name slots the compacted pool may have given to other
 *   nodes, so restore also requires every slot the file names to be all-zero still (always true for a pool that was
 *   never compacted: eviction zeroed them) and returns SVOSLAM_ERR_FORMAT, pool untouched, otherwise. */
int svoslam_pool_evict_subtree(svoslam_pool *pool, const uint8_t *path, int32_t levels, const char *file, void *stream);
int svoslam_pool_restore_subtree(svoslam_pool *pool, const char *file, void *stream);
int svoslam_subtree_file_nodes(const char *file, uint32_t **h_words, int32_t *num_nodes);
/* graft: the way back in that does not depend on node numbering.  The file is validated as by restore (magic, length,
 *   checksum, relative child indices); its path is walked in the pool (SVOSLAM_ERR_INVALID_ARG if it leaves the tree, or
 *   if the node has children: the cube was fused into meanwhile); the file's tiles are APPENDED at base = pool->size
 *   (the pool grows if it has to; SVOSLAM_ERR_POOL_LIMIT beyond 2^30 nodes) with child indices base + relative index,
 *   the node gets FLAG | base and keeps its colour word.  The file's node_index, pool_size and tile indices are not
 *   looked at, so it works on compacted and never-compacted pools alike (on the latter the tree equals restore's, the
 *   numbering does not).  Also SVOSLAM_ERR_INVALID_ARG when a plan of the structure chain is ahead of its commit or a
 *   deferred commit waits for its apply: their splits take the same indices behind pool->size.  The pool grows as for
 *   a fusion (at least doubling), so grafting into a pool that was shrunk to fit undoes the shrink.  Blocking. */
int svoslam_pool_graft_subtree(svoslam_pool *pool, const char *file, void *stream);
/* Compacting re-index: the pool becomes exactly the tiles reachable from the root tile (nodes 0..7) in CANONICAL ORDER --
 * breadth-first from tile 0, each level in the order of the parent nodes' new indices, then octant 0..7: the rule evict
 * uses below a node, applied from the root -- so two pools that hold the same tree hold the same bytes afterwards.
 * Colour words and word0 of childless nodes are copied, word0 of a node with children becomes FLAG | 8 * (new index of
 * its child tile); tiles nothing points to (zeroed by an eviction, or anything else) are dropped.  size becomes
 * 8 * (reachable tiles), the device-resident size follows, pending / pending_bound become 0.
 * Out of place: the nodes move to a fresh allocation and the old one is freed -- capacity_nodes <= 0 keeps the present
 * capacity, otherwise the new capacity is max(capacity_nodes, size_after): this is how memory is handed back.  Peak
 * device use is the old plus the new allocation; when capacity_nodes is smaller than size_before the new allocation
 * is first sized for size_before (all that is known before the walk) and trimmed by one device copy, so the transient
 * peak of that form is old + size_before + trimmed.  The march acceleration data follows the pool and is rebuilt in
 * full by the next render; the shadow words of deferred commits (8 bytes per node of capacity, allocated by the first
 * svo_fuse_commit_deferred) are released when the capacity shrank and allocated anew, for the new capacity, by the next
 * deferred commit.  The next fusion or graft that does not fit grows the pool as ever (at least doubling).
 * d_old_tile (optional, device, size_before / 8 entries): entry k = the old first-node index of the tile that became
 * new tile k.
 * SVOSLAM_ERR_INVALID_ARG: a plan of the structure chain is ahead of its commit, or a deferred commit waits for its
 * apply (compacting between the two is not allowed: the same rule as for save and resize).  A plain svo_fuse_plan
 * without its commit yet does not stop the compaction but is void afterwards -- the workspace holds node indices of the
 * old numbering --: svo_fuse_commit* and svo_fuse_split_early then return SVOSLAM_ERR_INVALID_ARG; plan again.
 * SVOSLAM_ERR_FORMAT: a
 * child index that is not a multiple of 8 or lies outside size_before, or more tiles visited than size_before / 8 (a
 * cycle or a shared tile in a foreign pool).  On any error the pool is untouched.  Blocking: waits for the whole device. */
typedef struct {
  int32_t size_before, size_after;         /* nodes */
  int32_t capacity_before, capacity_after; /* nodes */
  int32_t levels;                          /* tile levels visited, root tile = level 0 */
  int32_t tiles_dropped;                   /* (size_before - size_after) / 8 */
} svoslam_compact_stats;
int svoslam_pool_compact(svoslam_pool *pool, int32_t capacity_nodes, uint32_t *d_old_tile, svoslam_compact_stats *stats,
                         void *stream);
/* dst becomes a byte-identical replica of src (nodes, size, at least src's capacity); dst may be zero-initialised.
 * Blocking (waits for the device). */
int svoslam_pool_copy(svoslam_pool *dst, svoslam_pool *src, void *stream);
int svoslam_pool_load(svoslam_pool *pool, const char *path, float center[3], float *edge_length, int32_t *max_depth,
                      void *stream);

/* Opaque scratch arena reused across calls (sort buffers, plan records...).
 * The reference cudaMallocs ~6+D temporaries per call instead. */
typedef struct svoslam_workspace svoslam_workspace;
int svoslam_workspace_create(svoslam_workspace **ws);
int svoslam_workspace_destroy(svoslam_workspace *ws);

/* per-call statistics of the fusion path (host, filled after the call) */
typedef struct {
  int32_t num_points;       /* n */
  int32_t num_split;        /* nodes split = new tiles allocated */
  int32_t pass_sizes[SVOSLAM_MAX_DEPTH + 1]; /* code_sizes[] of svo.cu:179-237 */
  int32_t pool_size_before;
  int32_t pool_size_after;
} svoslam_fuse_stats;

/* replaces svo::svoFromPointCloud (include/octree_slam/world/svo/svo.h:16,
 * src/world/svo/svo.cu:642-696).  d_points: n x vec3, d_colors: n x 3 bytes
 * (Color256).  center/edge_length = root centre and HALF edge.
 * Blocking once (one 4-byte count readback, as the reference's `int&
 * octree_size` requires the new size on the host). stats may be NULL. */
int svoslam_svo_from_point_cloud(svoslam_workspace *ws, const float *d_points, const uint8_t *d_colors,
                                 int32_t n, int32_t max_depth, svoslam_pool *pool, const float center[3],
                                 float edge_length, svoslam_fuse_stats *stats, void *stream);

/* Same fusion, fully asynchronous: nothing is read back, the new size stays on the device
 * (pool->d_size) and pool->size becomes exact again at the next blocking call or svoslam_pool_sync.
 * Capacity is reserved ahead for the worst case (sum over levels of min(8^d, n) splits per call);
 * only when that reservation runs out does the call synchronise once to learn the true size. */
int svoslam_svo_from_point_cloud_async(svoslam_workspace *ws, const float *d_points, const uint8_t *d_colors,
                                       int32_t n, int32_t max_depth, svoslam_pool *pool, const float center[3],
                                       float edge_length, void *stream);

/* The asynchronous fusion in its three phases, for callers that overlap it with a render of the
 * previous state (svoFromPointCloud then coneTraceSVO per frame, src/main.cpp:44,56):
 *   sort   keys + sort of the points; touches only the workspace
 *   plan   reads the pool's tree (must follow the previous commit; may run while the pool is ray-marched)
 *   commit writes the pool (splits, leaf blend, mip levels) and consumes the plan
 * sort -> plan -> commit on one workspace == svoslam_svo_from_point_cloud_async.  Fusions in flight at
 * the same time need a workspace each.  If plan has to grow the pool it first waits for the whole device. */
int svoslam_svo_fuse_sort(svoslam_workspace *ws, const float *d_points, int32_t n, int32_t max_depth,
                          const float center[3], float edge_length, void *stream);
/* The sort phase fed by a raw depth frame: generateVertexMap (image_kernels.cu:24-58), transformVertexMap by the
 * DEVICE-resident mat4 d_pose (main.cpp:40-41), computePointCloudBoundingBox (image_kernels.cu:60-102; main.cpp:43) and
 * computeKeys (svo.cu:33-66) in ONE launch, without a point cloud in memory, then the sort: same sorted keys as
 * generate_vertex_map -> transform_vertex_map_dmat -> point_cloud_bbox_device -> svo_fuse_sort.  d_bbox7 (optional) =
 * {min xyz, max xyz, any}.  Needs 3 max_depth + 1 + ceil(log2(width height)) <= 64 (SVOSLAM_ERR_INVALID_ARG otherwise). */
int svoslam_svo_fuse_sort_frame(svoslam_workspace *ws, const uint16_t *d_depth, const float *d_pose, int32_t width, int32_t height,
                                float fx, float fy, int32_t max_depth, const float center[3], float edge_length, float *d_bbox7,
                                void *stream);
int svoslam_svo_fuse_plan(svoslam_workspace *ws, int32_t n, int32_t max_depth, svoslam_pool *pool, void *stream);
int svoslam_svo_fuse_commit(svoslam_workspace *ws, const uint8_t *d_colors, int32_t n, int32_t max_depth,
                            svoslam_pool *pool, void *stream);
/* Sorted keys from elsewhere (frame-sharded sessions, DESIGN.md section 5: the rank that owns a frame sorts it and the sorted
 * arrays are all-gathered): _export_sorted copies the outcome of this workspace's sort phase to d_keys_out[n] (ascending
 * Morton keys, invalid points = 1) and d_idx_out[n] (point index per key; equal keys in ascending index order: R1);
 * _adopt_sorted makes such arrays the outcome of a workspace's sort phase -- svoslam_svo_fuse_plan / _split_early /
 * _commit follow as after svoslam_svo_fuse_sort.  The adopted arrays stay the caller's and must stay valid until the
 * commit has run.  Replaces nothing in the reference (svo.cu:602 sorts every cloud where it is fused). */
/* Row bands ("each GPU computes keys for its band ... all-gather of the sorted lists, merge -> identical global
 * list on every rank -> identical newNode = num_nodes + 8 x rank"): _sort_frame_band is svoslam_svo_fuse_sort_frame for rows
 * [first_row, first_row + rows) of the image, with whole-image point indices; _merge_sorted merges `lists` (<= 16) sorted
 * (key, index) lists with ascending, disjoint index ranges (bands in order) into d_keys_out / d_idx_out, which then hold
 * exactly what one sort of the whole frame produces: adopt them (below), plan, commit. */
int svoslam_svo_fuse_sort_frame_band(svoslam_workspace *ws, const uint16_t *d_depth, const float *d_pose, int32_t width, int32_t height,
                                     float fx, float fy, int32_t max_depth, const float center[3], float edge_length, int32_t first_row,
                                     int32_t rows, void *stream);
int svoslam_svo_fuse_merge_sorted(const unsigned long long *const *d_keys, const uint32_t *const *d_idx, const int32_t *counts, int32_t lists,
                                  unsigned long long *d_keys_out, uint32_t *d_idx_out, void *stream);
int svoslam_svo_fuse_export_sorted(svoslam_workspace *ws, int32_t n, unsigned long long *d_keys_out, uint32_t *d_idx_out, void *stream);
int svoslam_svo_fuse_adopt_sorted(svoslam_workspace *ws, const unsigned long long *d_keys, const uint32_t *d_idx, int32_t n, int32_t max_depth);
/* Optional, between plan and commit (same workspace, same pool, direct commit only): initialises the child tiles of the
 * planned splits (splitNodes' tile writes, svo.cu:239-276) beyond the pool's present size -- nothing a ray march of the pool
 * can reach -- so that it may run WHILE the previous frame is still being rendered; the commit then writes the links from
 * its leaf kernel and runs two launches instead of three.  Same pool contents as without the call. */
int svoslam_svo_fuse_split_early(svoslam_workspace *ws, int32_t n, int32_t max_depth, svoslam_pool *pool, void *stream);
/* The structure chain, for callers that do NOT render every frame (one rank of a frame-sharded session).  A plan reads only
 * the tree's structure words, and those are final once the previous frame's splits are in (splitNodes, svo.cu:239-276); its
 * leaf blend and mip levels (fillNodes / mipmapNodes, :291-465) write colour words only.  plan_structure = plan + all splits
 * with their links, tiles numbered from a size that follows the plans; it waits for no commit, only for the previous
 * plan_structure (same stream, or ordered by the caller).  The commits (svoslam_svo_fuse_commit on the same workspace: leaf
 * kernel + straddlers) follow in frame order on another stream.  The caller must keep a render of frame k away from the
 * structure of frame k+1: no plan_structure(k+1) before the render of frame k has finished.  pool_structure_begin: once per
 * sequence, ordered after everything earlier on the pool.  Same pool contents as plan + commit per frame. */
int svoslam_pool_structure_begin(svoslam_pool *pool, void *stream);
int svoslam_svo_fuse_plan_structure(svoslam_workspace *ws, int32_t n, int32_t max_depth, svoslam_pool *pool, void *stream);
/* The commit in two halves, for callers that ray-march the map while the next frame is being fused (the frame
 * scheduler): svoslam_svo_fuse_commit_deferred does all the work of the commit -- splitNodes, fillNodes, mipmapNodes,
 * svo.cu:239-465 -- without a store a concurrent cone trace of the pool in its present state can observe (new tiles
 * lie beyond the pool's size, colour words go to a shadow array of 8 bytes per node of capacity, the links of the
 * first-pass split nodes wait); svoslam_svo_fuse_apply (same workspace, before it is used again; any stream ordered
 * after the deferred call AND after the last reader of the old state) publishes it in one short launch.  Between the
 * two the pool may be read (old state) but not fused into, saved or resized; one deferred commit per pool at a time.
 * deferred + apply == svoslam_svo_fuse_commit, byte for byte. */
int svoslam_svo_fuse_commit_deferred(svoslam_workspace *ws, const uint8_t *d_colors, int32_t n, int32_t max_depth,
                                     svoslam_pool *pool, void *stream);
int svoslam_svo_fuse_apply(svoslam_workspace *ws, svoslam_pool *pool, void *stream);
/* Key-range sharded fusion: the plan + commit of ONE frame (splitKeys .. mipmapNodes, svo.cu:179-465) cut across `world` ranks by key range
 * instead of being replicated on every rank (the reference is single-GPU, cuda_renderer.cpp:68; protocol:
 * tests/test_keyrange_gloo.py).  Every rank holds a byte-identical replica of the pool and the frame's sorted keys (svoslam_svo_fuse_sort* +
 * export / merge).  Per frame and rank: keyrange_commit plans and commits the rank's slice -- the keys under a contiguous run of level-3
 * octree cells holding about n / world keys; every rank computes the same cuts -- where no replica can see it yet and writes the rank's
 * DELTA into d_delta (delta_bytes of room; 64 bytes per key of the slice is ample): bucket sizes, new tiles, frontier links, {node,
 * colour word} of the existing nodes it changed, records the receivers' ray-march marks need.  The caller all-gathers the deltas
 * (word 10 of a delta = the number of 32-bit words that carry data).  keyrange_apply (same workspace) renumbers every rank's tiles into the
 * reference's order (pass-major, depth, key), writes all deltas -- the own one included -- to their global place, makes the marks of the
 * level grid / occupancy bricks from all keys, recomputes the colour words above the splitter level and sets the pool's size: the replica
 * is then byte-identical to a pool that fused the frame in one piece.  d_deltas: HOST array of `world` device pointers in rank order.
 * Frames whose splits reach above level 3 (a node of level 1 or 2 without children: the first frames of a map) make several ranks plan the
 * same records: the deltas list those by key and the apply ranks them in the ranks' union -- no special case for the caller.
 * keyrange_status (blocking; optional, e.g. once per call of a frame loop): 0, or why an apply did NOT happen -- until it has been
 * read every later apply on the workspace is refused as well (a replica that silently missed a frame must not go on).
 * world <= 16, max_depth >= 6. */
#define SVOSLAM_KEYRANGE_OVERFLOW 2  /* a delta did not fit its buffer */
#define SVOSLAM_KEYRANGE_MISMATCH 4  /* deltas of different frames / pool states */
#define SVOSLAM_KEYRANGE_USED_WORD 10
int svoslam_svo_fuse_keyrange_commit(svoslam_workspace *ws, const unsigned long long *d_sorted_keys, const uint32_t *d_sorted_idx,
                                     const uint8_t *d_colors, int32_t n, int32_t max_depth, svoslam_pool *pool, int32_t rank, int32_t world,
                                     uint32_t *d_delta, int64_t delta_bytes, void *stream);
int svoslam_svo_fuse_keyrange_apply(svoslam_workspace *ws, const unsigned long long *d_sorted_keys, int32_t n, int32_t max_depth, svoslam_pool *pool,
                                    const uint32_t *const *d_deltas, int32_t world, void *stream);
int svoslam_svo_fuse_keyrange_status(svoslam_workspace *ws, int32_t *flags, void *stream);
/* instead of keyrange_apply: the delta was wanted, the commit is dropped (the pool stays as it was, the plan's reservation is released) */
int svoslam_svo_fuse_keyrange_discard(svoslam_workspace *ws, svoslam_pool *pool);

/* replaces svo::svoFromVoxelGrid (svo.h:14, svo.cu:584-640).  d_centers,
 * d_colors: n x vec4 (VoxelGrid, common_types.h:55-63). */
int svoslam_svo_from_voxel_grid(svoslam_workspace *ws, const float *d_centers, const float *d_colors, int32_t n,
                                int32_t max_depth, svoslam_pool *pool, const float center[3], float edge_length,
                                svoslam_fuse_stats *stats, void *stream);

/* replaces svo::extractVoxelGridFromSVO (svo.h:18, svo.cu:699-745).  On return
 * *d_centers / *d_colors are hipMalloc'ed n x vec4 arrays owned by the caller
 * (free with svoslam_free), *n_out the voxel count.  Blocking. */
int svoslam_extract_voxel_grid(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth,
                               const float center[3], float edge_length, float **d_centers, float **d_colors,
                               int32_t *n_out, void *stream);
int svoslam_free(void *d_ptr);

/* The map's surface at max_depth as a welded quad mesh (no reference counterpart; specification in DESIGN.md section 12).
 * Cells: exactly those svoslam_extract_voxel_grid(pool, max_depth) returns -- every node on the path has alpha > 127, every
 * node above the cell has children; below the fused depth the mip alpha gives a coarser surface.  With x, y, z in [0, N),
 * N = 2^max_depth, read off the cell's octants (bit 0 = x, 1 = y, 2 = z), a face of a cell is emitted iff the cell behind it
 * is outside [0, N)^3 or not occupied.  Faces are ordered by (cell in extraction order, direction -x +x -y +y -z +z); a face
 * is four vertex indices, counter-clockwise seen from outside, and the cell's colour word unchanged (R | G<<8 | B<<16 | A<<24).
 * Vertices are welded: one per lattice corner (ix, iy, iz) in [0, N]^3 that a face uses, ascending in
 * iz << 2(max_depth+1) | iy << (max_depth+1) | ix.  Position per axis, in binary32, one division, one multiplication and one
 * addition in this order:   center + (float)(2 i - N) * (edge_length / (float)N)      (edge_length = half edge, as everywhere)
 * -- NOT the halved-and-summed centres svoslam_extract_voxel_grid computes level by level: a cell's corners are in general
 * not bit-equal to that call's centre -/+ half a cell.
 * Blocking.  Outputs are hipMalloc'ed and owned by the caller (svoslam_free): 3 floats per vertex, 4 indices per face, one colour
 * per face; all NULL and *stats all 0 for an empty surface.  A pool with pending asynchronous fusions is handled as by
 * svoslam_extract_voxel_grid (the stream is drained first; pool->size == 0, an uninitialised pool, returns the empty surface
 * before that: an initialised pool holds at least its 8 root children, also while its size lags).  Errors: that call's argument and depth errors;
 * SVOSLAM_ERR_POOL_LIMIT when 4 x faces exceeds 2^31 - 1.  On any error nothing is left allocated. */
typedef struct { int32_t cells, faces, vertices; } svoslam_surface_stats;
int svoslam_extract_surface_mesh(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const float center[3],
                                 float edge_length, float **d_vertices, uint32_t **d_quads, uint32_t **d_face_colors,
                                 svoslam_surface_stats *stats, void *stream);
/* Host only, needs no device: writes a mesh (host arrays) as binary little-endian PLY 1.0 -- vertex x y z float; face = a
 * uchar-counted list of uint vertex indices, then uchar red green blue alpha.  triangulate != 0 writes two triangles
 * (0,1,2), (0,2,3) per quad, both with the quad's colour.  SVOSLAM_ERR_INVALID_ARG for an index >= n_vertices (nothing is
 * written), SVOSLAM_ERR_IO when the file cannot be written (a partial file is removed). */
int svoslam_mesh_write_ply(const char *path, const float *h_vertices, int32_t n_vertices, const uint32_t *h_quads,
                           const uint32_t *h_face_colors, int32_t n_faces, int32_t triangulate);
/* Asking the map (no reference counterpart; specification in DESIGN.md section 13).  Both calls work on any pool, the library's
 * own or foreign words (svoslam_pool_set_nodes), take n inputs in device memory and write caller-allocated device arrays of n
 * entries, every output pointer optional (NULL: not written).  Neither allocates or reads anything back; both are asynchronous
 * on `stream`, except that a pool with pending asynchronous fusions is drained first, as by svoslam_extract_voxel_grid.  A pool
 * whose deferred commit waits for its apply is seen as a renderer sees it: in its old state.  One ray or point per lane in the
 * caller's order: coherent neighbours (rays of one view, points of one scan) are faster than shuffled ones.
 * Errors: SVOSLAM_ERR_INVALID_ARG for n < 0, max_depth outside [1, SVOSLAM_MAX_DEPTH], !(edge_length > 0), NULL center, and with
 * n > 0 a NULL pool, an uninitialised pool or NULL inputs.  n == 0 is SVOSLAM_OK and launches nothing.
 *
 * svoslam_pool_cast_rays: the first occupied cell along each ray, by exact traversal -- no step length, nothing is jumped.
 *   Occupied set: exactly the cells svoslam_extract_voxel_grid(pool, max_depth) returns and svoslam_extract_surface_mesh wraps
 *     -- every node on the path at levels 1..d has alpha > 127, every node at levels 1..d-1 has children; a childless node above
 *     d contributes nothing; a d below the fused depth casts against the mip alpha.
 *   Geometry: the mesh's lattice, so hits lie on mesh faces.  N = 2^d, h = edge_length / (float)N; plane k (0..N) of axis a is
 *     P_a(k) = center_a + (float)(2k - N) * h; cell x spans P(x)..P(x+1).  All arithmetic is binary32, every product and sum
 *     rounded on its own, in the order written.
 *   Ray: d_rays holds origin o then direction v (6 floats per ray; v need not be a unit vector), a point is o + t v, and
 *     r_a = 1.0f / v_a once per ray for v_a != 0.  The parameter of a plane is (P_a(k) - o_a) * r_a.
 *   Cell of a coordinate: c_a(p) = the number of k in 1..N-1 with P_a(k) <= p; with v_a < 0 the comparison is <, so a point on a
 *     plane belongs to the cell it is moving into.
 *   Start: with P_a(0) <= o_a <= P_a(N) on all axes the origin is inside: cell (c_x(o_x), c_y(o_y), c_z(o_z)), t = 0, face 6.
 *     Otherwise per axis with v_a != 0 the near and far root planes are 0 and N (swapped for v_a < 0); t_enter is the largest
 *     near parameter, the entry axis the lowest that attains it; a miss if t_enter < 0, if t_enter exceeds the smallest far
 *     parameter, or if an axis with v_a == 0 has o_a outside the root.  The entry axis starts at 0 or N-1, the others at
 *     c_b(o_b + t_enter * v_b); t = t_enter.
 *   Step: walk the current cell's path from the root.  The first node with alpha <= 127, or without children above level d, at
 *     level l frees its aligned block of 2^(d-l) cells per axis [lo, hi]; reaching level d with alpha > 127 is the hit.  From a
 *     free block: the parameter of the leaving plane (hi+1 for v_a > 0, lo for v_a < 0) of each axis with v_a != 0; the smallest
 *     wins, the lowest axis on a tie (no parameter below +inf: a miss).  That axis moves to the first cell beyond the block --
 *     outside [0, N) the ray has left the root: a miss.  Each other coordinate becomes c_b of the point at that parameter,
 *     clamped to the block's range on b, and never moves backwards against the sign of v_b.  t = max(t, that parameter).  A t
 *     above t_max is a miss, here and at the start.  At most 3N steps (every coordinate is monotone, one advances strictly).
 *   d_t_max: n floats, or NULL for unlimited.
 *   Outputs: d_t the entry parameter of the hit cell (+inf: miss; NaN: invalid ray -- a non-finite component or v == 0 -- which
 *     does no traversal); d_node the level-d node (-1: no hit); d_cell = x | y << 16 | z << 32 | face << 48, face the direction
 *     id of the face entered as in svoslam_extract_surface_mesh (-x +x -y +y -z +z = 0..5: v_x > 0 enters through 0), 6 = the
 *     origin was inside the cell (all ones: no hit); d_color the node's colour word (0: no hit); d_steps the blocks visited,
 *     the hit block included.
 *
 * svoslam_pool_query_points: the node that holds each point (d_points: 3 floats per point), by the FUSION's descent -- octant
 *   bits from p > c, the edge halved, the centre moved by +-edge (computeKey) -- to max_depth or the first childless node, so a
 *   point that was fused is found in its own leaf.  A point with !(center_a - edge_length <= p_a <= center_a + edge_length) on
 *   any axis is outside (a NaN by the same test).  The ray cast is tied to the mesh's planes, the lookup to the fusion's halved-
 *   and-summed centres: the two boundaries of a cell differ by float rounding only, as the mesh's vertices and the voxel
 *   grid's centres do.
 *   Outputs: d_node (-1: outside), d_level (the node's level, 1..max_depth; 0: outside), d_key (a leading 1, then one octant
 *   triple per level walked: the fusion's key format; 0: outside), d_color (the node's colour word; 0: outside). */
int svoslam_pool_cast_rays(const svoslam_pool *pool, int32_t max_depth, const float center[3], float edge_length, const float *d_rays,
                           const float *d_t_max, int32_t n, float *d_t, int32_t *d_node, uint64_t *d_cell, uint32_t *d_color,
                           uint32_t *d_steps, void *stream);
int svoslam_pool_query_points(const svoslam_pool *pool, int32_t max_depth, const float center[3], float edge_length,
                              const float *d_points, int32_t n, int32_t *d_node, int32_t *d_level, uint64_t *d_key, uint32_t *d_color,
                              void *stream);
/* Asking the map by volume (no reference counterpart; specification here and in DESIGN.md section 14).  Both calls follow the
 * conventions of svoslam_pool_cast_rays above: any pool, n inputs in device memory, caller-allocated device arrays of n entries,
 * every output pointer optional, nothing allocated or read back, asynchronous on `stream` except that pending asynchronous
 * fusions are drained first, a pool whose deferred commit waits for its apply seen in its old state, the same argument errors,
 * n == 0 is SVOSLAM_OK and launches nothing.  One box or point per lane in the caller's order.
 *   Common: d = max_depth, N = 2^d; the occupied set at d, the planes P_a(k) = center_a + (float)(2k - N) * (edge_length /
 *     (float)N) and the count c_a(p) = the number of k in 1..N-1 with P_a(k) <= p (strict form: <) are svoslam_pool_cast_rays'.
 *     The Morton code m of a cell interleaves the bits of x, y, z with x lowest (octant = x | y << 1 | z << 2 per level: the octant
 *     of level l is bits 3(d-l)..3(d-l)+2 of m).  The block of level l around m is the aligned cube of 2^(d-l) cells per axis:
 *     the Morton range [m with its low 3(d-l) bits cleared, that + 8^(d-l)).
 *   The walk over an inclusive cell range [lo, hi] (it defines `steps`): next_in(m) is the smallest Morton code >= m whose cell
 *     lies in [lo, hi] (pure integer geometry, nothing is loaded).  Start at m = morton(lo).  Repeat: m = next_in(m); stop if
 *     m > morton(hi); count one step and descend from the root along m's path, l = 1..d: the node is loaded; alpha <= 127, or
 *     l < d and no children, frees the block of level l: m = the block's end; at l == d the cell is occupied: visit it, m += 1.
 *     Free space costs one step per block of the tree, as in the ray cast.
 *
 * svoslam_pool_count_boxes: the occupied cells in each axis-aligned box (d_boxes: 6 floats per box, min xyz then max xyz).
 *   Box to cells: a box with a NaN component, with min_a > max_a, or with max_a < P_a(0) or min_a > P_a(N) on any axis is empty:
 *     count 0, first_cell all ones, first_node -1, steps 0.  Infinities are allowed (-inf..+inf: the whole axis).  Otherwise
 *     lo_a = c_a(min_a) and hi_a = max(lo_a, strict c_a(max_a)): a box face on a lattice plane does not take in the cell beyond.
 *   Visit: count += 1; the first visit records first_cell = x | y << 16 | z << 32 and first_node (the level-d node): the lowest
 *     occupied cell in Morton order.  stop_after > 0 ends the walk as soon as count == stop_after (1: the any-hit collision
 *     test); <= 0 is unlimited.
 *   Outputs: d_count, d_first_cell, d_first_node, d_steps (descents).
 *
 * svoslam_pool_nearest_occupied: the nearest occupied cell within radius_cells (R, 0..SVOSLAM_MAX_RADIUS_CELLS, else
 *   SVOSLAM_ERR_INVALID_ARG: 3 R^2 fits an int32) of each point's cell (d_points: 3 floats per point), exactly, in integers.
 *   A point with a NaN or with !(P_a(0) <= p_a <= P_a(N)) on an axis gives dist2 -2, cell all ones, node -1, colour 0, steps 0.
 *   Otherwise q_a = c_a(p_a), the range is [max(q - R, 0), min(q + R, N - 1)], best = R^2 + 1, and the walk above runs with one
 *   more test at each level of the descent, before the load: D = sum_a max(block_lo_a - q_a, 0, q_a - block_hi_a)^2 of the block
 *   of that level; D >= best skips the block exactly as a free one.  Visit: best = D of the cell = sum (x_a - q_a)^2 (< best by
 *   the test), and the cell, node and colour word are recorded; the walk ends when best == 0.
 *   Outputs: d_dist2 the squared centre-to-centre distance in cells to the nearest occupied cell within R, among equally near
 *     cells the lowest in Morton order (-1: none within R; the distance in metres is sqrt(dist2) * 2 * edge_length / N), d_cell =
 *     x | y << 16 | z << 32 (all ones: none), d_node (-1: none), d_color (0: none), d_steps descents, however a descent ends. */
#define SVOSLAM_MAX_RADIUS_CELLS 4096
int svoslam_pool_count_boxes(const svoslam_pool *pool, int32_t max_depth, const float center[3], float edge_length, const float *d_boxes,
                             int64_t stop_after, int32_t n, uint64_t *d_count, uint64_t *d_first_cell, int32_t *d_first_node,
                             uint32_t *d_steps, void *stream);
int svoslam_pool_nearest_occupied(const svoslam_pool *pool, int32_t max_depth, const float center[3], float edge_length,
                                  const float *d_points, int32_t radius_cells, int32_t n, int32_t *d_dist2, uint64_t *d_cell,
                                  int32_t *d_node, uint32_t *d_color, uint32_t *d_steps, void *stream);
/* The distance field of a map region (no reference counterpart; specification here and in DESIGN.md section 15): for every cell of
 * a box of cells, the squared distance in cells to the nearest occupied cell if that is within radius_cells, exactly, in integers
 * -- an Euclidean distance transform truncated at R.  The dense form of svoslam_pool_nearest_occupied: neighbouring cells share
 * almost all of their answer, so the occupied cells of the region are rasterised once and three separable passes follow.
 *   Occupied set: d = max_depth (1..SVOSLAM_MAX_DEPTH), N = 2^d; the occupied set at d is svoslam_pool_cast_rays': the cells
 *     svoslam_extract_voxel_grid(pool, d) lists (below the fused depth the mip alpha decides; a childless node above d
 *     contributes nothing).  A cell that is not in it is free.
 *   Region: the cells q with origin_cell_a <= q_a < origin_cell_a + dims_a, in cells at depth d.  It has to lie inside the root:
 *     0 <= origin_cell_a and origin_cell_a + dims_a <= N.  There is no centre and no edge length: once the occupied set is known
 *     everything is integers.
 *   Output: d_dist2, dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest: index ((z - oz) * ny + (y - oy)) *
 *     nx + (x - ox).  With R = radius_cells (0..SVOSLAM_MAX_RADIUS_CELLS) the value at q is the minimum of (cx - qx)^2 + (cy - qy)^2
 *     + (cz - qz)^2 over ALL occupied cells c of the root -- those outside the region too -- if that minimum is <= R^2, and -1
 *     otherwise: exactly the dist2 svoslam_pool_nearest_occupied returns for a point inside cell q with the same d and R.  Metres
 *     are sqrt(dist2) * 2 * edge_length / N.  Only the value is specified, not how it is computed.
 *   Conventions: those of the calls above.  Any pool (foreign words set with svoslam_pool_set_nodes included); asynchronous on
 *     `stream`, nothing is read back; pending asynchronous fusions are drained first, as svoslam_extract_voxel_grid drains them;
 *     a pool whose deferred commit waits for its apply is seen in its old state.  Intermediates (the occupancy of the region
 *     inflated by R as bit rows, and the field after the x and the y pass) live in grow-only slots of the workspace: a call that
 *     needs more than the workspace has allocates, a second call of the same size does not.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG: ws,
 *     origin_cell or dims NULL; max_depth outside 1..SVOSLAM_MAX_DEPTH; a negative entry of dims; a region not inside the root;
 *     radius_cells outside 0..SVOSLAM_MAX_RADIUS_CELLS; with a non-empty region a NULL or uninitialised pool or a NULL d_dist2.
 *     SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1 output cells, or an intermediate of more than 2^31 - 1 elements (the inflated region
 *     at a large R can reach that).  SVOSLAM_ERR_OOM: an allocation failed; nothing the call allocated stays behind on an error.
 *
 * svoslam_box_to_cells (host only, needs no device): the inclusive cell range [lo, hi] of an axis-aligned box (min xyz then max xyz)
 *   at max_depth, by svoslam_pool_count_boxes' "Box to cells" above, the same planes and counts in the same binary32 operations:
 *   lo_a = c_a(min_a), hi_a = max(lo_a, strict c_a(max_a)); *empty = 1 for a box with a NaN component, with min_a > max_a, or with
 *   max_a < P_a(0) or min_a > P_a(N) on any axis (lo and hi are still written), else 0.  The values lie in [0, N): the field of the
 *   box one would hand to svoslam_pool_count_boxes is origin_cell = lo, dims = hi - lo + 1.  SVOSLAM_ERR_INVALID_ARG: a NULL
 *   pointer, max_depth outside 1..SVOSLAM_MAX_DEPTH, !(edge_length > 0). */
int svoslam_pool_distance_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                                const int32_t dims[3], int32_t radius_cells, int32_t *d_dist2, void *stream);
int svoslam_box_to_cells(int32_t max_depth, const float center[3], float edge_length, const float box[6], int32_t lo[3], int32_t hi[3],
                         int32_t *empty);
/* profiling form of svoslam_pool_distance_field: the same call and the same result, but BLOCKING, with an event before the first
 * launch and after each of the four: launch_ms = the milliseconds of the raster, the x pass, the y pass and the z pass (zeros when
 * nothing is launched; NULL: SVOSLAM_ERR_INVALID_ARG).  For tools/map_field_bench.py; each event costs its stream a few
 * microseconds. */
int svoslam_pool_distance_field_profile(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                                        const int32_t dims[3], int32_t radius_cells, int32_t *d_dist2, float launch_ms[4], void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's three distance-field slots (the bit rows, the field after
 * the x pass, after the y pass; NULL / 0 before the first call): what a test of "a second call of the same size does not allocate"
 * looks at.  Host only. */
int svoslam_workspace_field_buffers(const svoslam_workspace *ws, void *d_ptrs[3], uint64_t bytes[3]);
/* The reach field of a map region (no reference counterpart; specification here and in DESIGN.md section 16): for every cell of a
 * box of cells, the number of face-neighbour moves of the shortest path from any seed cell that stays in traversable cells of the
 * region -- a cost-to-go field (navigation function, wavefront).  Exact, in integers.
 *   d, N, the occupied set and the region are exactly those of svoslam_pool_distance_field: cells at depth d = max_depth, the
 *     region origin_cell .. origin_cell + dims inside the root.
 *   Traversable set T: with r = clearance_cells (0..SVOSLAM_MAX_RADIUS_CELLS) a region cell q is traversable iff no occupied cell
 *     of the WHOLE root lies within squared distance r^2 of it -- exactly the condition under which svoslam_pool_distance_field
 *     with radius_cells = r writes -1 at q.  Occupied cells up to r outside the region block cells inside it; at r = 0 an occupied
 *     cell itself is blocked.
 *   Seeds: d_seeds, n_seeds triples (x, y, z) of int32 absolute cells at depth d, in device memory.  A seed counts if it lies in
 *     the region and is in T; any other seed is ignored (negative or >= N included).  Duplicates are allowed.  n_seeds = 0 is
 *     allowed, and d_seeds may then be NULL.
 *   Output: d_steps, dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest, indexed as d_dist2 is.  The
 *     value at q is -2 if q is not in T; otherwise the number of moves of the shortest path from any counted seed to q, where a
 *     move goes to one of the six face neighbours and every cell of the path is in T and IN THE REGION (0 at a counted seed); -1
 *     if there is no such path.  Metres along the path = steps * 2 * edge_length / N.  Only these values are specified, not how
 *     they are computed.  stats (may be NULL): seeds_used = the seed entries that counted, duplicates counted each; rounds and
 *     tile_runs are diagnostics with no specified value (the launches of the relaxation and the tiles they worked on).
 *   Conventions: those of svoslam_pool_distance_field -- any pool; pending asynchronous fusions are drained first; a deferred
 *     commit's pool is read in its old state; the intermediates (the distance field's, the traversable bit rows and the tile flags)
 *     live in grow-only slots of the workspace, so a second call of the same size allocates nothing -- with ONE DIFFERENCE: THE CALL
 *     BLOCKS.  The relaxation runs in rounds and the host reads one small convergence record (32 bytes) per round, as
 *     svoslam_extract_surface_mesh reads back once per level; after the last round's readback the finishing launch is
 *     asynchronous on `stream`, like the output of every other call.  The result does not depend on scheduling.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_distance_field (clearance_cells for radius_cells, d_steps for d_dist2), n_seeds < 0, NULL d_seeds with
 *     n_seeds > 0.  SVOSLAM_ERR_POOL_LIMIT: the limits of svoslam_pool_distance_field with radius_cells = clearance_cells, or more than
 *     2^24 - 1 tiles of 64 x 8 x 8 cells (a region one cell wide in x with ny * nz near 2^31), decided before anything is allocated
 *     or written.  SVOSLAM_ERR_OOM: an allocation failed; the slots the call grew are released.
 *     SVOSLAM_ERR_HIP with a text in svoslam_last_error: the round cap (tiles * cells per tile + 1) was reached, which the
 *     argument of section 16 rules out. */
typedef struct { int32_t rounds, tile_runs, seeds_used; } svoslam_reach_stats;
int svoslam_pool_reach_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                             const int32_t dims[3], int32_t clearance_cells, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_steps,
                             svoslam_reach_stats *stats /* may be NULL */, void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's two reach-field slots (the traversable bit rows; the
 * control record with the tile flags; NULL / 0 before the first call), as svoslam_workspace_field_buffers shows the distance
 * field's.  Host only. */
int svoslam_workspace_reach_buffers(const svoslam_workspace *ws, void *d_ptrs[2], uint64_t bytes[2]);
/* The component labels of a map region (no reference counterpart; specification here and in DESIGN.md section 17): for every cell of
 * a box of cells that belongs to a set S, a label that names its connected component of S inside the region, and optionally that
 * component's size -- "are A and B connected at all" is labels[a] == labels[b], "drop floaters under k cells" is sizes >= k.
 * Exact, in integers.
 *   d, N, the occupied set and the region are exactly those of svoslam_pool_distance_field: cells at depth d = max_depth, the
 *     region origin_cell .. origin_cell + dims inside the root.
 *   The set S: with r = clearance_cells (0..SVOSLAM_MAX_RADIUS_CELLS), T is svoslam_pool_reach_field's traversable set: the region
 *     cells where svoslam_pool_distance_field with radius_cells = r writes -1.  which = SVOSLAM_COMPONENTS_FREE: S = T.  which =
 *     SVOSLAM_COMPONENTS_SOLID: S = the region's cells that are not in T -- at r = 0 the occupied cells of the region, at r > 0 the
 *     occupied cells dilated by r (occupied cells up to r outside the region count).
 *   Components: two cells of S are connected iff a chain of face-neighbour moves joins them whose every cell is in S AND IN THE
 *     REGION.  Connectivity is 6, as in the reach field: cells that touch only by an edge or a corner are not connected by that
 *     contact.  A caller who wants looser clustering of occupied cells asks for SOLID with r = 1, which joins cells up to two
 *     apart; 26-connectivity is not offered.
 *   Output: d_labels, dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest, indexed as d_dist2 is.  The
 *     value at q is -1 if q is not in S; otherwise the SMALLEST OUTPUT INDEX of any cell of q's component.  The labels are
 *     therefore canonical: labels[labels[q]] == labels[q], labels[q] <= q, and the result does not depend on scheduling.
 *     d_sizes (may be NULL): the same shape; at every cell of S the number of cells of its component, elsewhere 0.  stats (may be
 *     NULL): components = the number of components; largest = the size of the largest one, 0 if d_sizes is NULL or S is empty;
 *     tile_passes and unions are diagnostics with no specified value (the sweeps inside tiles, the links made across tile
 *     faces).  Only these values are specified, not how they are computed.
 *   Conventions: those of svoslam_pool_distance_field -- any pool; pending asynchronous fusions are drained first; a deferred
 *     commit's pool is read in its old state; the intermediates (the distance field's, the bit rows of S and a 32-byte control
 *     record) live in grow-only slots of the workspace, so a second call of the same size allocates nothing.  THE CALL IS
 *     ASYNCHRONOUS ON `stream` WHEN stats IS NULL: nothing is read back, there are no rounds.  With stats it blocks for one
 *     readback of the control record at the end.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_distance_field (clearance_cells for radius_cells, d_labels for d_dist2), or `which` outside {0, 1}.
 *     SVOSLAM_ERR_POOL_LIMIT: the limits of svoslam_pool_distance_field with radius_cells = clearance_cells, or more than 2^24 - 1
 *     tiles of 64 x 8 x 8 cells, decided before anything is allocated or written.  SVOSLAM_ERR_OOM: an allocation failed; the
 *     slots the call grew are released, after the stream has drained. */
#define SVOSLAM_COMPONENTS_FREE  0
#define SVOSLAM_COMPONENTS_SOLID 1
typedef struct { int32_t components, largest, tile_passes, unions; } svoslam_component_stats;
int svoslam_pool_label_components(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                                  const int32_t dims[3], int32_t clearance_cells, int32_t which, int32_t *d_labels,
                                  int32_t *d_sizes /* may be NULL */, svoslam_component_stats *stats /* may be NULL */, void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's two component slots (the bit rows of S; the control
 * record; NULL / 0 before the first call), as svoslam_workspace_reach_buffers shows the reach field's.  Host only. */
int svoslam_workspace_component_buffers(const svoslam_workspace *ws, void *d_ptrs[2], uint64_t bytes[2]);
/* The nearest-cell field of a map region (no reference counterpart; specification here and in DESIGN.md section 18): for every cell
 * of a box of cells the squared distance to the nearest cell of a target set AND that cell, the witness -- what the gradient of a
 * distance field, a Voronoi skeleton, "which obstacle is nearest" (labels[witness] of svoslam_pool_label_components) and the colour
 * of an offset surface are made of, and what cannot be rebuilt from the distances without searching again.  Exact, in integers.
 *   d, N, the occupied set, the region, the output order (x fastest) and R = radius_cells (0..SVOSLAM_MAX_RADIUS_CELLS) are exactly
 *     those of svoslam_pool_distance_field.
 *   Target set A: which = SVOSLAM_NEAREST_OCCUPIED: the occupied cells of the whole root.  which = SVOSLAM_NEAREST_FREE: the cells
 *     of the root that are not occupied; nothing outside the root is a cell, so a fully occupied root has an empty A.  Target cells
 *     up to R outside the region count, as they do for the distance field.
 *   Value at q: D = the minimum of (cx - qx)^2 + (cy - qy)^2 + (cz - qz)^2 over c in A.  If D > R^2, or A is empty: dist2 = -1,
 *     cell = all ones, node = -1, color = 0.  Otherwise dist2 = D and cell = x | y << 16 | z << 32 of the witness: the cell of A at
 *     squared distance D with the SMALLEST z, THEN THE SMALLEST y, THEN THE SMALLEST x, in absolute cell coordinates.  For OCCUPIED
 *     dist2 equals svoslam_pool_nearest_occupied's (for a point inside cell q) and svoslam_pool_distance_field's.  The tie rule is
 *     NOT svoslam_pool_nearest_occupied's lowest Morton code: the cell can differ from that call's, but only among equally near
 *     cells.  (It is the rule three separable passes give when each prefers the lower coordinate.)  The signed distance of an ESDF
 *     is +sqrt(dist2 OCCUPIED) at a free cell and -sqrt(dist2 FREE) at an occupied one.
 *   d_node, d_color: for OCCUPIED the level-d node of the witness and its colour word, what svoslam_pool_cast_rays reports for that
 *     cell.  For FREE both must be NULL: a free cell has no level-d node in general.
 *   Outputs: d_dist2, d_cell, d_node, d_color, each dims[0] * dims[1] * dims[2] values in device memory, indexed as
 *     svoslam_pool_distance_field's d_dist2.  Every one of them may be NULL; with a non-empty region not all.  Only the values are
 *     specified, not how they are computed.
 *   Conventions: those of svoslam_pool_distance_field -- any pool (svoslam_pool_set_nodes words included); asynchronous on `stream`,
 *     nothing is read back; pending asynchronous fusions are drained first; a pool whose deferred commit waits for its apply is
 *     read in its old state.  The intermediates live in three grow-only workspace slots of their own (the bit rows of A on the
 *     inflated region; the values after the x, y and z pass; one 16-bit index per pass), so a second call of the same size
 *     allocates nothing, and the distance field's slots are never touched.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_distance_field; `which` outside {0, 1}; FREE with a d_node or d_color; with a non-empty region all four
 *     outputs NULL.  SVOSLAM_ERR_POOL_LIMIT: under svoslam_pool_distance_field's conditions, decided before anything is allocated.
 *     SVOSLAM_ERR_OOM: an allocation failed; nothing the call grew stays behind. */
#define SVOSLAM_NEAREST_OCCUPIED 0
#define SVOSLAM_NEAREST_FREE     1
int svoslam_pool_nearest_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                               const int32_t dims[3], int32_t radius_cells, int32_t which, int32_t *d_dist2 /* may be NULL */,
                               uint64_t *d_cell /* may be NULL */, int32_t *d_node /* may be NULL */, uint32_t *d_color /* may be NULL */,
                               void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's three nearest-cell slots (the bit rows; the values; the
 * indices; NULL / 0 before the first call), as svoslam_workspace_field_buffers shows the distance field's.  Host only. */
int svoslam_workspace_nearest_buffers(const svoslam_workspace *ws, void *d_ptrs[3], uint64_t bytes[3]);
/* The visibility field of a map region (no reference counterpart; specification here and in DESIGN.md section 19): for every cell
 * of a box of cells the viewpoints that have a free line of sight to it within a range -- what coverage ("which cells did these
 * poses see"), next-best-view and sensor placement, line-of-sight pruning of a path from the reach field and visibility graphs
 * between waypoints are made of.  Exact, in integers, symmetric, the same on every machine.
 *   d, N, the occupied set, the region and the output order (x fastest, [nz, ny, nx]) are exactly those of
 *     svoslam_pool_distance_field.  R = range_cells, 0..SVOSLAM_MAX_RADIUS_CELLS.
 *   Viewpoints: d_views holds n_views triples (x, y, z) of int32 absolute cells at depth d, in device memory, as the reach field's
 *     seeds are.  Viewpoint k COUNTS iff it lies in the root (0 <= v_a < N on every axis); it need not lie in the region, and
 *     whether its own cell is occupied is ignored.  A viewpoint that does not count sees nothing.  Its bit keeps its position k:
 *     bits are never renumbered.  Duplicates are allowed.  n_views = 0 is allowed, d_views may then be NULL, and the outputs are
 *     all zero.
 *   Sight: for cells v and q of the root let S(v, q) be the set of cells c, c != v and c != q, whose CLOSED cube [c, c + 1]^3 meets
 *     the closed segment from v's centre to q's centre: the supercover of the segment without its two ends.  q is SEEN FROM v iff
 *     |q - v|^2 <= R^2 and no cell of S(v, q) is occupied.  The rule is geometric, so sight is symmetric in v and q.  A segment
 *     that touches an occupied cell only at an edge or a corner is blocked -- the conservative choice: no line of sight through a
 *     crack of zero width; it deliberately differs from whatever tie rule svoslam_pool_cast_rays has.  An occupied q can be seen (a
 *     sensor sees the surface cell); q == v is always seen; at R = 0 a viewpoint sees its own cell and nothing else.  Everything is
 *     integers: in doubled coordinates the centres are odd and the cell faces even; with D = q - v the segment crosses axis a's
 *     i-th face at parameter (2 i - 1) / (2 |D_a|); two crossings compare by cross-multiplication, (2 i - 1) |D_b| against
 *     (2 j - 1) |D_a|, which stays below 2^25 at R = 4096; where two or three axes cross at the same parameter the segment passes
 *     through an edge or a corner and all 4 or 8 cells around it belong to the supercover.
 *   Outputs: each dims[0] * dims[1] * dims[2] values in device memory, indexed as svoslam_pool_distance_field's d_dist2.  Either may
 *     be NULL; with a non-empty region not both.  d_mask (uint32): bit k is set iff viewpoint k counts and q is seen from it; it
 *     needs n_views <= SVOSLAM_MAX_VIEWS_MASK.  d_count (int32): the number of viewpoint entries that count and see q, duplicates
 *     counted each; any n_views.  Only the values are specified, not how they are computed.
 *   Conventions: those of svoslam_pool_distance_field -- any pool (svoslam_pool_set_nodes words included); asynchronous on `stream`,
 *     nothing is read back; pending asynchronous fusions are drained first; a pool whose deferred commit waits for its apply is
 *     read in its old state.  The one intermediate, the occupancy of the region inflated by R and clipped to the root as bit rows,
 *     lives in one grow-only workspace slot of its own, so a second call of the same size allocates nothing, and no other call's
 *     slots are touched.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_distance_field, with range_cells for radius_cells; n_views < 0; NULL d_views with n_views > 0; d_mask
 *     with n_views > SVOSLAM_MAX_VIEWS_MASK; with a non-empty region both outputs NULL.  SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1
 *     output cells or bit-row words, decided before anything is allocated or written.  SVOSLAM_ERR_OOM: the allocation failed;
 *     nothing the call grew stays behind.
 *   Not part of it: a field-of-view cone or sensor model per viewpoint, the first blocker of each line, sub-cell viewpoints. */
#define SVOSLAM_MAX_VIEWS_MASK 32
int svoslam_pool_visibility_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                                  const int32_t dims[3], int32_t range_cells, const int32_t *d_views, int32_t n_views,
                                  uint32_t *d_mask /* may be NULL */, int32_t *d_count /* may be NULL */, void *stream);
/* diagnostics: the device pointer and size in bytes of the workspace's visibility slot (the bit rows; NULL / 0 before the first
 * call), as svoslam_workspace_field_buffers shows the distance field's.  Host only. */
int svoslam_workspace_visibility_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);
/* Viewpoints that cover a map region (no reference counterpart; specification here and in DESIGN.md section 24): out of n_cands
 * places to stand, which few see the most of a set of target cells, and what is still unseen after them -- the question of an
 * inspection or exploration planner, answered in one call: a compacted target list, a candidate-by-target bit matrix under
 * svoslam_pool_visibility_field's sight rule, and a greedy set cover over it.  Exact, in integers, ties decided, all on the device.
 *   d, N, the occupied set, the region and the order of a per-cell array (x fastest, [nz, ny, nx]) are exactly those of
 *     svoslam_pool_distance_field.  R = range_cells, 0..SVOSLAM_MAX_RADIUS_CELLS.
 *   Targets: a region cell is a target iff it passes target_mode and, where d_select is not NULL, its byte there is non-zero
 *     (d_select: one uint8 per region cell in device memory, in region order).  SVOSLAM_COVER_SURFACE: the cell is occupied and at
 *     least one of its six face neighbours lies in the root and is not occupied; a neighbour outside the region still counts, a
 *     neighbour outside the root does not.  SVOSLAM_COVER_FREE: the cell is not occupied.  SVOSLAM_COVER_ALL: every cell.  Targets
 *     are numbered in region order; T is their number.
 *   Candidates: d_cands holds n_cands triples (x, y, z) of int32 absolute cells at depth d, in device memory, as
 *     svoslam_pool_visibility_field's d_views.  A candidate COUNTS iff it lies in the root; it need not lie in the region, and
 *     whether its own cell is occupied is ignored.  One that does not count sees nothing.  Duplicates are allowed; indices are
 *     never renumbered.
 *   Sight: svoslam_pool_visibility_field's rule, word for word: candidate c sees target q iff |q - v_c|^2 <= R^2 and no cell of
 *     S(v_c, q) is occupied; edges and corners block, q == v is seen, an occupied q can be seen.
 *   Scores: d_seen[c] = the number of targets c sees, 0 if it does not count.
 *   Greedy cover: `covered` starts empty.  In round j = 0, 1, ...: gain(c) = the number of targets c sees that are not yet covered;
 *     the round takes the candidate with the largest gain, among equal gains the LOWEST INDEX; if that gain is < min_gain, or
 *     j == k_max, the cover ends; otherwise d_chosen[j] = c, d_gain[j] = gain, and the targets c sees become covered.  Entries past
 *     the end are d_chosen = -1 and d_gain = 0.  min_gain >= 1; k_max is 0..SVOSLAM_MAX_COVER_VIEWS; k_max = 0 gives the scores and
 *     the summary only, and d_chosen / d_gain may then be NULL.
 *   d_round: one int32 per region cell: -1 not a target; -2 a target that no chosen candidate sees; otherwise the round j whose
 *     candidate first covered it.  d_summary: four int32 (T, n_chosen, covered, coverable); coverable = the number of targets that
 *     at least one candidate sees.  Only the values are specified, not how they are computed.
 *   Conventions: those of svoslam_pool_visibility_field -- any pool; pending asynchronous fusions are drained first; a pool whose
 *     deferred commit waits for its apply is read in its old state.  ONE THING DIFFERS: the call reads T back once (4 bytes) to
 *     size the matrix, so it blocks until the target list is ranked, as svoslam_pool_reach_field blocks for its rounds; everything
 *     after that readback, all k_max rounds included, is queued without another.  The intermediates live in four grow-only
 *     workspace slots of their own (the occupancy bit rows of the region inflated by max(R, 1); flags / ranks and the target list;
 *     the matrix, n_cands * ceil(T / 64) words of 64 bits; the covered words and one record per round), so a second call of the same
 *     size allocates nothing, and no other call's slots are touched.
 *   Errors: a zero entry of dims is SVOSLAM_OK: it writes the entries past the end (all k_max of them) and a zero summary and
 *     nothing else.  T = 0 and n_cands = 0 are valid; d_cands may then be NULL.  SVOSLAM_ERR_INVALID_ARG: those of
 *     svoslam_pool_visibility_field that concern the region, the range and the candidates; target_mode outside 0..2; k_max outside
 *     0..SVOSLAM_MAX_COVER_VIEWS; min_gain < 1; NULL d_summary; NULL d_chosen or d_gain with k_max > 0 -- nothing is launched,
 *     written or allocated.  SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1 region cells or bit-row words, decided before anything is
 *     allocated; a matrix of more than 2^29 words (4 GiB), decided right after the readback of T, before the matrix is allocated
 *     and before any output is written -- what the call grew until then is released.  SVOSLAM_ERR_OOM: an allocation failed;
 *     nothing the call grew stays behind.
 *   Not part of it: a field-of-view cone or sensor model per candidate, weights per target, candidate poses rather than cells, an
 *     optimal rather than greedy cover, the matrix as an output. */
#define SVOSLAM_COVER_SURFACE 0
#define SVOSLAM_COVER_FREE    1
#define SVOSLAM_COVER_ALL     2
#define SVOSLAM_MAX_COVER_VIEWS 1024
int svoslam_pool_cover_views(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                             const int32_t dims[3], int32_t range_cells, int32_t target_mode, const uint8_t *d_select /* may be NULL */,
                             const int32_t *d_cands, int32_t n_cands, int32_t k_max, int32_t min_gain,
                             int32_t *d_seen /* n_cands, may be NULL */, int32_t *d_chosen /* k_max */, int32_t *d_gain /* k_max */,
                             int32_t *d_round /* region cells, may be NULL */, int32_t *d_summary /* 4 */, void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's four cover slots (the bit rows; flags / ranks and the
 * target list; the matrix; the covered words and round records; NULL / 0 before the first call), as
 * svoslam_workspace_visibility_buffers shows the visibility field's.  Host only. */
int svoslam_workspace_cover_buffers(const svoslam_workspace *ws, void *d_ptrs[4], uint64_t bytes[4]);
/* The observed space of a map region (no reference counterpart; specification here and in DESIGN.md section 25).  Every region
 * field above treats "not occupied" as "free"; these two calls tell a cell a sensor looked through from a cell nothing ever looked
 * at, beside the map: the pool, the fusion and every other call are untouched.  Together with svoslam_pool_cover_views they close
 * the loop of an exploring robot: observe, find the frontier of the known, choose the next views of it, plan to them.
 *
 * svoslam_field_observe_rays: what a set of sensor rays has seen
 *   Like svoslam_score_poses the call sees no pool.  d = max_depth, N = 2^d; the planes P_a(k) and the count c_a(p) are
 *     svoslam_pool_cast_rays' (center, edge_length as there).  The region has to lie inside the root, by
 *     svoslam_pool_distance_field's test.
 *   d_obs: one uint8 per region cell in device memory, x fastest ([nz, ny, nx]).  d_points: n_frames blocks of n triples of binary32
 *     in the sensor frame, frame f at d_points + 3 n f: what svoslam_generate_vertex_map writes.  d_poses: n_frames x 16 binary32,
 *     each a sensor-to-world matrix in the layout of every trans[16] of this header.
 *   One ray (frame f with pose M, point p), classified in this order:
 *     1. VOID if a component of p is not finite;
 *     2. otherwise o = (m[12], m[13], m[14]) and w = M * (p, 1) in binary32 in the operation order of
 *        svoslam_transform_vertex_map, no fused multiply-add: step 1 of svoslam_score_poses;
 *     3. OUTSIDE if a component of o or of w is not finite or fails the root test P_a(0) <= . <= P_a(N) on any axis;
 *     4. otherwise s_a = c_a(o_a) and e_a = c_a(w_a), the non-strict count svoslam_pool_nearest_occupied gives a point;
 *     5. with D = e - s: FAR if range_cells > 0 and |D|^2 > range_cells^2 (compared in 64 bits); range_cells = 0 is no limit,
 *        the valid range is 0..2^SVOSLAM_MAX_DEPTH.  A far ray is skipped whole, not truncated;
 *     6. otherwise MARKED: e gets SVOSLAM_OBS_END; if s != e, s and every cell of S(s, e) get SVOSLAM_OBS_THROUGH, S being the
 *        supercover without its ends of svoslam_pool_visibility_field (edges and corners touched count).  Only cells of the region
 *        are stored; a MARKED ray whose cells all lie outside the region marks nothing and still counts as MARKED.
 *   The result is a set: it does not depend on the order of rays, lanes or frames.  accumulate == 0: d_obs[q] = the marks of this
 *     call, its other bits 0.  accumulate != 0: d_obs[q] |= the marks; bits 2..7 are left as found.
 *   d_summary: six int64 in device memory (void, outside, far, marked, cells_through, cells_end); the last two count the region
 *     cells whose bit is set in d_obs AFTER the call.  May be NULL.  Nothing is read back; everything is queued on `stream`.
 *   Workspace: the two bit planes over the region's rows live in one grow-only slot of their own; the six counts are added
 *     straight into d_summary.  A second call of the same size allocates nothing, no other call's slot is touched.
 *   Errors: a zero entry of dims is SVOSLAM_OK: it writes the summary's four ray counts (every non-void ray in the root and in
 *     range is MARKED) and zero cell counts.  n == 0 or n_frames == 0 is valid: d_obs is cleared, or left unchanged under
 *     accumulate.  SVOSLAM_ERR_INVALID_ARG: NULL ws, center, origin_cell or dims; max_depth outside 1..SVOSLAM_MAX_DEPTH;
 *     !(edge_length > 0); a negative entry of dims; a region not inside the root; n < 0; n_frames < 0; range_cells outside
 *     0..2^SVOSLAM_MAX_DEPTH; NULL d_obs with a non-empty region; NULL d_points or d_poses with n * n_frames > 0.
 *     SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1 region cells, or n * n_frames > 2^31 - 1.  SVOSLAM_ERR_OOM: the allocation
 *     failed.  On an error nothing is launched, written or allocated, and what the call grew is released.
 *   Not part of it: changing the pool; truncating a long ray at the range; rays with an end outside the root; ray counts per cell;
 *     a noise model.
 *
 * svoslam_pool_frontier_field: the observation held against the map
 *   d, N, the occupied set, the region and the order are exactly those of svoslam_pool_distance_field.  d_obs as above; T is a
 *     cell's THROUGH bit, E its END bit, the other bits are ignored.  The state of a cell:
 *       SVOSLAM_STATE_UNKNOWN   not occupied, neither bit
 *       SVOSLAM_STATE_FREE      not occupied, T, not E
 *       SVOSLAM_STATE_FRONTIER  FREE, and at least one of its six face neighbours lies in the REGION and is UNKNOWN
 *       SVOSLAM_STATE_OCCUPIED  occupied, and not (T without E)
 *       SVOSLAM_STATE_VACATED   occupied, T, not E: rays passed through it and none ended in it -- evidence, not proof: a grazing
 *                               ray touches a wall's cells too
 *       SVOSLAM_STATE_UNMAPPED  not occupied, E
 *     A neighbour outside the region never makes a frontier: its state is not known to the call.
 *   Outputs, each may be NULL, not all three: d_state, one uint8 per region cell; d_frontier, 1 iff the state is FRONTIER, else 0:
 *     directly svoslam_pool_cover_views' d_select; d_summary, six int32: the number of cells per state.
 *   Conventions: those of svoslam_pool_visibility_field -- any pool; pending asynchronous fusions are drained first; a pool whose
 *     deferred commit waits for its apply is read in its old state; nothing is read back.  The one intermediate, the occupancy of
 *     the region itself as bit rows, lives in one grow-only workspace slot of its own.
 *   Errors: those of svoslam_pool_visibility_field for the region (a zero entry of dims is SVOSLAM_OK and writes a zero summary);
 *     SVOSLAM_ERR_INVALID_ARG also for NULL d_obs with a non-empty region and for all three outputs NULL.
 *   Not part of it: frontier clustering; a frontier across the region's border; thresholds on counts. */
#define SVOSLAM_OBS_THROUGH 1
#define SVOSLAM_OBS_END     2
#define SVOSLAM_STATE_UNKNOWN  0
#define SVOSLAM_STATE_FREE     1
#define SVOSLAM_STATE_FRONTIER 2
#define SVOSLAM_STATE_OCCUPIED 3
#define SVOSLAM_STATE_VACATED  4
#define SVOSLAM_STATE_UNMAPPED 5
int svoslam_field_observe_rays(svoslam_workspace *ws, uint8_t *d_obs, int32_t max_depth, const float center[3], float edge_length,
                               const int32_t origin_cell[3], const int32_t dims[3], const float *d_points, int32_t n,
                               const float *d_poses, int32_t n_frames, int32_t range_cells, int32_t accumulate,
                               int64_t *d_summary /* 6, may be NULL */, void *stream);
int svoslam_pool_frontier_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                                const int32_t dims[3], const uint8_t *d_obs, uint8_t *d_state /* may be NULL */,
                                uint8_t *d_frontier /* may be NULL */, int32_t *d_summary /* 6, may be NULL */, void *stream);
/* diagnostics: the device pointer and size in bytes of the workspace's observation slot (the two bit planes) and of its frontier
 * slot (the bit rows; NULL / 0 before the first call), as svoslam_workspace_visibility_buffers shows the visibility field's.  Host
 * only. */
int svoslam_workspace_observe_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);
int svoslam_workspace_frontier_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);
/* The owner field of a map region (no reference counterpart; specification here and in DESIGN.md section 26): the reach field's
 * steps and, for every reached cell, WHICH seed is nearest by path -- a partition of free space among seeds (robots sharing a
 * frontier, the nearest dock, rooms grown back from their cores: `segment_rooms` of the Python package).  Exact, in integers.
 *   d, N, the occupied set, the region and the traversable set T are exactly svoslam_pool_reach_field's: T = the region cells where
 *     svoslam_pool_distance_field with radius_cells = clearance_cells writes -1.  Moves go to the six face neighbours, inside T
 *     and inside the region.
 *   Seeds, list form (d_seed_field == NULL): d_seeds, n_seeds triples (x, y, z) as in svoslam_pool_reach_field.  An entry counts
 *     iff it lies in the region and in T; duplicates are allowed; the label of entry k is k.  n_seeds = 0 is allowed, and d_seeds
 *     may then be NULL.
 *   Seeds, field form (d_seed_field != NULL; d_seeds must then be NULL and n_seeds 0): d_seed_field is an int32 per region cell,
 *     indexed as the outputs are.  A cell is a seed iff its value v satisfies 0 <= v < 2^31 - 1 and the cell is in T; its label is
 *     v.  d_seed_field == d_owner is allowed, so a label field is grown in place: every cell's label is read before the cell is
 *     written.  Any other overlap between arguments is the caller's error.
 *   Outputs: d_steps and d_owner, each dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest, indexed as
 *     d_dist2 is.  d_steps is exactly what svoslam_pool_reach_field writes for the counted seeds: -2 not in T, -1 no path,
 *     otherwise the shortest number of moves.  d_owner is, at a cell with steps >= 0, the SMALLEST LABEL AMONG THE COUNTED SEEDS
 *     WHOSE SHORTEST PATH TO THE CELL HAS EXACTLY `steps` MOVES; elsewhere the value of d_steps (-1 or -2).  A seed cell that
 *     carries several list entries takes the smallest index.  The tie rule is over all shortest paths, not the first to arrive:
 *     the result does not depend on scheduling.  Only these values are specified, not how they are computed.
 *   stats (may be NULL): seeds_used = the counted seed entries (list form, duplicates counted each) or seed cells (field form);
 *     rounds, tile_runs (the steps' relaxation) and owner_rounds, owner_tile_runs (the owners') are diagnostics with no specified
 *     value.
 *   Conventions: those of svoslam_pool_reach_field -- pending asynchronous fusions are drained first; a deferred commit's pool is
 *     read in its old state; THE CALL BLOCKS, with one 32-byte readback per round of either relaxation; one SVOSLAM_STAGE_QUERY
 *     bracket around everything.  No slot of its own: d_steps and d_owner are the working arrays, the reach field's two slots hold
 *     T's rows and the control record with the tile flags (one more int per tile than the reach field asks), so a second call of
 *     the same size allocates nothing.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_reach_field; both seed forms given (d_seed_field with a non-NULL d_seeds or n_seeds != 0); with a
 *     non-empty region a NULL d_steps or d_owner, or d_steps == d_owner.  SVOSLAM_ERR_POOL_LIMIT, SVOSLAM_ERR_OOM and
 *     SVOSLAM_ERR_HIP: as svoslam_pool_reach_field, the limits decided before anything is allocated or written. */
typedef struct { int32_t rounds, tile_runs, seeds_used, owner_rounds, owner_tile_runs; } svoslam_owner_stats;
int svoslam_pool_owner_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                             const int32_t dims[3], int32_t clearance_cells, const int32_t *d_seeds, int32_t n_seeds,
                             const int32_t *d_seed_field /* NULL: list form */, int32_t *d_steps, int32_t *d_owner,
                             svoslam_owner_stats *stats /* may be NULL */, void *stream);
/* Scoring candidate poses against a distance field (no reference counterpart; specification here and in DESIGN.md section 20): for
 * each of n_poses sensor-to-world matrices, move each of n sensor points by it, look the point's cell up in the field of a region
 * and add the values up -- the inner loop of a likelihood-field or chamfer relocaliser ("where in this map was this depth frame
 * taken?"), in one launch instead of a transform, a nearest-cell query and a readback per pose.  The sums are integers: exact,
 * the same on every machine and in every order of summation.
 *   The field: d_dist2 is dims[0] * dims[1] * dims[2] int32 in device memory, x fastest, exactly as svoslam_pool_distance_field
 *     writes it for (max_depth, origin_cell, dims); svoslam_pool_nearest_field's dist2 serves as well.  A value >= 0 is a squared
 *     distance in cells, a negative value means "none within the radius".  The call sees neither the pool nor the radius.  The
 *     region has to lie inside the root, by svoslam_pool_distance_field's test.  d = max_depth, N = 2^d; the planes P_a(k) and the
 *     count c_a(p) are svoslam_pool_cast_rays' (center, edge_length as there).
 *   Points: d_points holds n triples of binary32 in the sensor frame, in device memory: what svoslam_generate_vertex_map writes,
 *     at any pyramid level.  A point with a non-finite component is VOID and counts nowhere (the vertex map writes +inf for a
 *     pixel without depth).
 *   Poses: d_poses holds n_poses x 16 binary32 in device memory, each a sensor-to-world matrix in the layout of every trans[16] of
 *     this header (column-major, m[4 * col + row]).
 *   One (pose M, point p) pair, p not void:
 *     1. w = M * (p, 1) in binary32, in the operation order of svoslam_transform_vertex_map: w_r = (m[r] * p.x + m[4 + r] * p.y) +
 *        (m[8 + r] * p.z + m[12 + r] * 1.0f), no fused multiply-add.
 *     2. the pair is OUTSIDE if a component of w is not finite;
 *     3. OUTSIDE if !(P_a(0) <= w_a <= P_a(N)) on any axis: the root test of svoslam_pool_nearest_occupied;
 *     4. otherwise q_a = c_a(w_a), the non-strict count: the cell svoslam_pool_nearest_occupied gives the point;
 *     5. OUTSIDE if q is not in the region;
 *     6. otherwise v = d_dist2[q]: the pair is FAR if v < 0 and NEAR if v >= 0.
 *   Per pose: cost = the sum of v over the NEAR pairs + miss_cost * (FAR + OUTSIDE), in int64; near, far, outside = the three
 *     counts, near + far + outside = the number of non-void points.  The natural miss_cost is R^2 + 1 of the field; any value in
 *     0..2^30 is allowed.
 *   Best: d_best is 2 x int64 = (cost, index) of the pose with the smallest cost among those with near >= min_near, among equal
 *     costs the lowest index; (-1, -1) if no pose qualifies, n_poses == 0 included.
 *   Outputs: d_cost (n_poses int64), d_near, d_far, d_outside (n_poses int32 each), d_best, all in device memory.  Each may be
 *     NULL; with n_poses > 0 not all five.  All are written asynchronously on `stream`; nothing is read back.  Only the values are
 *     specified, not how they are computed.
 *   Workspace: intermediates (a record per pose, when d_best is wanted or the points of one pose are split over workgroups) live
 *     in one grow-only workspace slot of their own: a second call of the same size allocates nothing, no other call's slot is
 *     touched.
 *   Errors: n == 0, or no non-void point, is valid: every pose has cost 0 and counts 0.  n_poses == 0 is SVOSLAM_OK and launches
 *     at most the write of d_best.  A zero entry of dims is valid: every non-void pair is OUTSIDE.  SVOSLAM_ERR_INVALID_ARG: ws,
 *     center, origin_cell or dims NULL; max_depth outside 1..SVOSLAM_MAX_DEPTH; !(edge_length > 0); a negative entry of dims; a
 *     region not inside the root; n < 0; n_poses < 0; miss_cost outside 0..2^30; min_near < 0; NULL d_points with n > 0; NULL
 *     d_poses with n_poses > 0; NULL d_dist2 with a non-empty region and n > 0 and n_poses > 0; all outputs NULL with n_poses > 0.
 *     SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1 region cells.  SVOSLAM_ERR_OOM: the allocation failed; nothing the call grew stays
 *     behind.  Nothing is launched on an error.
 *   Not part of it: setting a tracker's pose from the answer; normals or colour in the score; a sensor model for free space;
 *     sub-cell interpolation of the field. */
#define SVOSLAM_MAX_MISS_COST (1 << 30)
int svoslam_score_poses(svoslam_workspace *ws, const int32_t *d_dist2, int32_t max_depth, const float center[3], float edge_length,
                        const int32_t origin_cell[3], const int32_t dims[3], const float *d_points, int32_t n,
                        const float *d_poses, int32_t n_poses, int32_t miss_cost, int32_t min_near,
                        int64_t *d_cost, int32_t *d_near, int32_t *d_far, int32_t *d_outside, int64_t *d_best, void *stream);
/* diagnostics: the device pointer and size in bytes of the workspace's scoring slot (the per-pose records; NULL / 0 before the
 * first call that needs them), as svoslam_workspace_field_buffers shows the distance field's.  Host only. */
int svoslam_workspace_score_buffers(const svoslam_workspace *ws, void *d_ptrs[1], uint64_t bytes[1]);
/* Path planning in a map region (no reference counterpart; specification here and in DESIGN.md section 21): the reach field with a
 * weight per cell -- a cost-to-go field whose cheapest paths keep away from obstacles where they can, as the inflation layer in
 * front of every navigation stack's planner makes them -- and the paths themselves, traced down any such field for many starts at
 * once.  Exact, in integers.
 *
 * svoslam_pool_cost_field
 *   d, N, the occupied set, the region and the output order are exactly those of svoslam_pool_distance_field.
 *   Traversable set T and seeds: with r = clearance_cells (0..SVOSLAM_MAX_RADIUS_CELLS), T and the rule for which seeds count are
 *     exactly svoslam_pool_reach_field's: a region cell is in T iff no occupied cell of the WHOLE root lies within squared distance
 *     r^2 of it; a seed (d_seeds, n_seeds triples of int32 absolute cells, device memory) counts if it lies in the region and in T.
 *   Weight: R = comfort_cells, r <= R <= SVOSLAM_MAX_RADIUS_CELLS.  For q in T let D be the squared distance in cells to the nearest
 *     occupied cell of the whole root -- what svoslam_pool_distance_field with radius R writes, -1 meaning D > R^2.  If D > R^2,
 *     w(q) = 1.  Otherwise let j be the integer with (j - 1)^2 < D <= j^2, so r + 1 <= j <= R: w(q) = 1 + h_ring_cost[j - r - 1].
 *     h_ring_cost is HOST memory, R - r entries, each in 0..SVOSLAM_MAX_RING_COST; it may be NULL when R == r.  The profile need not
 *     be monotone.
 *   Output: d_cost, dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest, indexed as d_dist2 is.  The value
 *     at q is -2 if q is not in T; otherwise the minimum of the sum of w(p) over a path's cells EXCEPT ITS SEED, over the paths of
 *     face-neighbour moves from a counted seed to q whose every cell is in T and IN THE REGION: 0 at a counted seed, -1 if there is
 *     no such path.  Only these values are specified, not how they are computed; the result does not depend on scheduling.  With
 *     every ring cost 0, or with R == r, the field equals svoslam_pool_reach_field's d_steps value for value.  stats (may be NULL):
 *     seeds_used as in the reach field; max_weight = 1 + the largest ring cost (1 without rings); rounds and tile_runs are
 *     diagnostics with no specified value.
 *   Conventions: the reach field's -- any pool; pending asynchronous fusions are drained first; a deferred commit's pool is read in
 *     its old state; THE CALL BLOCKS, the host reads one small convergence record (32 bytes) per round; the intermediates (the
 *     distance field's, and three of its own: the bit rows of T, a 16-bit weight per cell, and the control record with the tile
 *     flags and the ring costs) live in grow-only slots of the workspace, so a second call of the same size allocates nothing.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG:
 *     those of svoslam_pool_reach_field (d_cost for d_steps), comfort_cells < clearance_cells or > SVOSLAM_MAX_RADIUS_CELLS, NULL
 *     h_ring_cost with R > r, an entry of it outside 0..SVOSLAM_MAX_RING_COST.  SVOSLAM_ERR_POOL_LIMIT, decided before anything is
 *     allocated or written: the limits of svoslam_pool_distance_field with radius_cells = R; more than 2^24 - 1 tiles of 64 x 8 x 8
 *     cells; n_out * max_weight >= 2^30 (the value of "not reached": a path has fewer cells than the region, so below this limit no
 *     finite cost can collide with it).  SVOSLAM_ERR_OOM: an allocation failed; the slots the call grew are released, after the
 *     stream has drained.  SVOSLAM_ERR_HIP with a text in svoslam_last_error: the round cap (tiles * cells per tile + 1) was
 *     reached, which the argument of section 21 rules out.
 *
 * svoslam_field_trace_paths (no pool, no workspace)
 *   d_field: any int32 array in device memory laid out as d_cost / d_steps over the region origin_cell .. origin_cell + dims.  A
 *     value >= 0 is a cost-to-go, a negative value means the cell cannot be entered.  d_starts: n_starts triples (x, y, z) of int32
 *     absolute cells, in device memory.
 *   The path of a start: if the start lies outside the region or its value is negative, the length is 0 and nothing is stored.
 *     Otherwise the path begins at the start; from a cell of value v > 0 it moves to a face neighbour INSIDE THE REGION whose value
 *     v' satisfies 0 <= v' < v, among those to the one with the smallest v', on a tie to the first in the order -x, +x, -y, +y, -z,
 *     +z; it ends at a cell of value 0.  On a field of svoslam_pool_cost_field or svoslam_pool_reach_field this is a cheapest /
 *     shortest path, and its cost summed by the field's own weights equals the value at the start.  The values fall strictly, so
 *     the walk is bounded by its data.
 *   Outputs: d_lengths[i] = the number of cells of the whole path, start and final cell included, EVEN WHEN IT EXCEEDS max_cells;
 *     d_paths [n_starts][max_cells][3] int32 receives the first min(length, max_cells) cells as absolute (x, y, z), the entries
 *     behind them are not written (d_paths may be NULL if max_cells == 0).  On an array that is not such a field the walk may reach
 *     a cell of value > 0 without a lower enterable neighbour: it stops there, and the length is MINUS the number of cells walked.
 *   Asynchronous on `stream`, nothing is read back.  All region arithmetic is in 64 bits.
 *   Errors: SVOSLAM_ERR_INVALID_ARG: NULL origin_cell or dims; a negative entry of dims, n_starts or max_cells; with n_starts > 0 a
 *     NULL d_starts or d_lengths, a NULL d_field with a non-empty region, a NULL d_paths with max_cells > 0.
 *     SVOSLAM_ERR_POOL_LIMIT: more than 2^31 - 1 cells, or n_starts * max_cells * 3 > 2^31 - 1.  A zero entry of dims gives lengths 0. */
#define SVOSLAM_MAX_RING_COST 65534
typedef struct { int32_t rounds, tile_runs, seeds_used, max_weight; } svoslam_plan_stats;
int svoslam_pool_cost_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                            const int32_t dims[3], int32_t clearance_cells, int32_t comfort_cells,
                            const int32_t *h_ring_cost /* HOST, comfort_cells - clearance_cells entries */, const int32_t *d_seeds,
                            int32_t n_seeds, int32_t *d_cost, svoslam_plan_stats *stats /* may be NULL */, void *stream);
int svoslam_field_trace_paths(const int32_t *d_field, const int32_t origin_cell[3], const int32_t dims[3], const int32_t *d_starts,
                              int32_t n_starts, int32_t max_cells, int32_t *d_paths /* [n_starts][max_cells][3], may be NULL if max_cells == 0 */,
                              int32_t *d_lengths /* [n_starts] */, void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's three cost-field slots (the bit rows of T; the weights;
 * the control record with the tile flags and the ring costs; NULL / 0 before the first call), as svoslam_workspace_reach_buffers
 * shows the reach field's.  Host only. */
int svoslam_workspace_plan_buffers(const svoslam_workspace *ws, void *d_ptrs[3], uint64_t bytes[3]);
/* Straightening planned paths (no reference counterpart; specification here and in DESIGN.md section 22): the clearance of straight
 * segments over a distance field -- the trajectory check, and the first blocker of a line -- and the pruning of a chain of cells,
 * such as svoslam_field_trace_paths writes, into a few vertices joined by straight segments that come no nearer to an obstacle
 * than the stretch of the chain they replace did.  Exact, in integers.  No pool, no workspace; asynchronous on `stream`, nothing
 * is read back; one SVOSLAM_STAGE_QUERY bracket around the one launch of each call.
 *
 * Common definitions
 *   d_dist2: int32 in device memory, dims[0] * dims[1] * dims[2] values, x fastest, over the region origin_cell .. origin_cell +
 *     dims, exactly as svoslam_pool_distance_field writes it: the squared distance in cells to the nearest occupied cell, -1 = none
 *     within the field's radius.
 *   g(c) = d_dist2[c] if that is >= 0, +infinity if it is -1, and 0 FOR A CELL OUTSIDE THE REGION (it counts as occupied).  No cell
 *     outside the region is read.
 *   C(a, b) for cells a and b: a, b and the supercover S(a, b) of svoslam_pool_visibility_field -- every other cell whose closed
 *     cube meets the closed segment between the two centres; edges and corners count.
 *   Walk order of C(a, b): a first; then the cells of S(a, b) crossing by crossing from a, where the segment passes through an edge
 *     or a corner first the side cells of one axis in x, y, z order, then those of two axes (xy, xz, yz), then the diagonal cell;
 *     b last.
 *   Limits: at most 2^16 cells per axis of the region (every region of a root is within it; the bound under which the walk's
 *     64-bit keys are proven, section 22) and at most 2^31 - 1 cells in all.
 *
 * svoslam_field_segment_clearance
 *   d_segments: n rows of 6 int32 in device memory, a (x, y, z) then b (x, y, z), absolute cells.  a == b is allowed (C = {a}); an
 *     end may lie outside the region, anywhere in int32: the minimum is then 0.
 *   Outputs: d_min[i] = the minimum of g over C(a_i, b_i), -1 when that is +infinity; so 0 means "touches an occupied cell or
 *     leaves the region".  d_at[i] (3 int32 per segment, may be NULL) = the first cell in walk order that attains the minimum,
 *     absolute; a when every cell is +infinity.  One lane per segment; a walk ends early only when 0 was reached.
 *   Errors: SVOSLAM_ERR_INVALID_ARG: NULL origin_cell or dims; a negative entry of dims or n; with n > 0 a NULL d_segments or d_min,
 *     a NULL d_dist2 with a non-empty region.  SVOSLAM_ERR_POOL_LIMIT: the limits above.  n == 0 launches nothing.  A zero entry of
 *     dims is valid: every cell has g = 0, d_min is 0 at a.
 *
 * svoslam_field_shorten_paths
 *   d_paths, d_lengths, n_paths, max_cells: exactly svoslam_field_trace_paths' outputs.  Path i has L = min(|d_lengths[i]|,
 *     max_cells) cells p_0 .. p_(L-1): a truncated path and a stopped (negative-length) one use their stored prefix.  The cells need
 *     not be face neighbours and need not lie in the region: any list of cells is accepted.
 *   r = clearance_cells, 0..SVOSLAM_MAX_RADIUS_CELLS.  THE CALLER MUST SUPPLY A FIELD WHOSE RADIUS IS >= r; the call cannot check it,
 *     and on a field of a smaller radius cells nearer than r pass for clear.  W = max_lookahead >= 0, 0 = unlimited.
 *   Rule: for a < j let m(a, j) = the minimum of g(p_i) over a <= i <= j.  The shortcut a -> j is admissible iff j == a + 1 (always,
 *     whatever the cells are), or every c of C(p_a, p_j) has g(c) > r^2 and g(c) >= m(a, j): the segment keeps the clearance and
 *     comes no nearer to an obstacle than the stretch it replaces was at its nearest.  The vertices are indices into the path: v_0
 *     = 0, then v_(k+1) = the LARGEST admissible j with v_k < j <= min(L - 1, v_k + W) (no upper window for W = 0), until L - 1 is
 *     reached.  Admissibility is not monotone in j; the whole window is examined.
 *   Outputs: d_counts[i] = the number of vertices, EVEN WHEN IT EXCEEDS max_vertices; 0 for L = 0, 1 for L = 1.  d_vertices
 *     [n_paths][max_vertices] int32 receives the first min(count, max_vertices) indices, the entries behind them are not written
 *     (d_vertices may be NULL if max_vertices == 0).
 *   With W = 1 every cell is a vertex.  On a field of radius r (every g > r^2 is +infinity) the rule is plain line-of-sight pruning
 *     at clearance r; on a field of svoslam_pool_cost_field's comfort radius a path stays in the rings it was planned through.
 *   Cost: one wavefront per path; with W = 0 a path of L cells takes O(L^2) walks in the worst case, W > 0 bounds it by L * W.
 *   Errors: SVOSLAM_ERR_INVALID_ARG: NULL origin_cell or dims; a negative entry of dims, n_paths, max_cells, max_lookahead or
 *     max_vertices; clearance_cells outside 0..SVOSLAM_MAX_RADIUS_CELLS; with n_paths > 0 a NULL d_lengths or d_counts, a NULL
 *     d_dist2 with a non-empty region, a NULL d_paths with max_cells > 0, a NULL d_vertices with max_vertices > 0.
 *     SVOSLAM_ERR_POOL_LIMIT: the limits above, n_paths * max_cells * 3 > 2^31 - 1, or n_paths * max_vertices > 2^31 - 1.  All are
 *     decided before anything is written.  n_paths == 0 launches nothing.  A zero entry of dims is valid: every cell has g = 0, so
 *     only the j == a + 1 steps remain. */
int svoslam_field_segment_clearance(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3],
                                    const int32_t *d_segments /* [n][6]: a xyz, b xyz */, int32_t n, int32_t *d_min /* [n] */,
                                    int32_t *d_at /* [n][3], may be NULL */, void *stream);
int svoslam_field_shorten_paths(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells,
                                const int32_t *d_paths /* [n_paths][max_cells][3] */, const int32_t *d_lengths /* [n_paths] */,
                                int32_t n_paths, int32_t max_cells, int32_t max_lookahead, int32_t max_vertices,
                                int32_t *d_vertices /* [n_paths][max_vertices], may be NULL if max_vertices == 0 */,
                                int32_t *d_counts /* [n_paths] */, void *stream);
/* Ground navigation in a map region (no reference counterpart; specification here and in DESIGN.md section 23): the cost-to-go
 * field of a robot that stands on surfaces -- support under it, headroom above it, a body radius measured above the bumps it can
 * roll over, a largest step it can climb and a price for climbing -- and the paths traced down it.  The ground counterpart of
 * svoslam_pool_cost_field and svoslam_field_trace_paths.  Exact, in integers; the result does not depend on scheduling.
 *
 * svoslam_pool_ground_field
 *   d, N, the occupied set O, the region and the output order are exactly those of svoslam_pool_distance_field.  Cells outside the
 *     root are not occupied.
 *   u: the unit cell vector of `up`: axis up >> 1 (1 = y, 2 = z), pointing to smaller coordinates if up & 1.  So 2 is +y (the
 *     project's convention), 3 -y, 4 +z, 5 -z.  0 and 1, the x axis, are SVOSLAM_ERR_INVALID_ARG: the bit rows run along x.
 *     "Horizontal" means the two axes other than u's; one of them is always x.
 *   Parameters: r = radius_cells, 0..SVOSLAM_MAX_RADIUS_CELLS; H = height_cells, 1..SVOSLAM_MAX_HEIGHT_CELLS; S = step_cells,
 *     0..min(H - 1, SVOSLAM_MAX_STEP_CELLS); c = climb_cost, 0..SVOSLAM_MAX_RING_COST; snap_cells, 0..SVOSLAM_MAX_SNAP_CELLS.
 *   Foothold set G: a region cell q is a foothold iff (1) q - u is a cell of the root and is occupied; (2) for k = 0 .. H - 1 the
 *     cell q + k u is not occupied; (3) for k = S .. H - 1 no occupied cell p exists that has the up-coordinate of q + k u and whose
 *     horizontal squared distance to q is at most r^2.  Occupied cells outside the region count: up to r horizontally, up to H - 1
 *     above and 1 below.  The body is a column of radius 0 up to the step height and a cylinder of radius r above it.  SUPPORT IS
 *     ASKED OF THE CENTRE CELL ONLY: a foothold may overhang an edge by up to r cells.
 *   Moves: from a foothold q to a foothold q + e + j u, e one of the four horizontal unit vectors, |j| <= S, both ends in the
 *     region.  A move costs 1 + c |j|.  No move is vertical.
 *   Seeds (d_seeds, n_seeds triples of int32 absolute cells, device memory): an entry outside the region is ignored.  Otherwise its
 *     foothold is the first cell of G met going from the seed against u, the seed itself first, at most snap_cells further cells
 *     examined, never leaving the region; an entry without one is ignored.
 *   Output: d_cost, dims[0] * dims[1] * dims[2] values of type int32 in device memory, x fastest, indexed as d_dist2 is: -2 where q
 *     is not in G, 0 at the foothold of a counted seed, otherwise the least total cost of a chain of moves from one, -1 without a
 *     chain.  stats (may be NULL): footholds = |G| (a specified value); seeds_used = the entries that found a foothold, duplicates
 *     each; rounds and tile_runs are diagnostics with no specified value.
 *   Conventions: svoslam_pool_cost_field's -- any pool; pending asynchronous fusions are drained first; a deferred commit's pool is
 *     read in its old state; THE CALL BLOCKS, the host reads one small record (32 bytes) per round; one SVOSLAM_STAGE_QUERY bracket;
 *     the intermediates live in six grow-only slots of the workspace (svoslam_workspace_ground_buffers), so a second call of the
 *     same size allocates nothing.
 *   Errors: a zero entry of dims is SVOSLAM_OK and launches nothing, if the other arguments are valid.  SVOSLAM_ERR_INVALID_ARG: a
 *     NULL ws, origin_cell or dims, max_depth outside 1..SVOSLAM_MAX_DEPTH, a region not inside the root, `up` outside 2..5, a
 *     parameter outside its range above, n_seeds < 0 or NULL d_seeds with n_seeds > 0; with a non-empty region a NULL or
 *     uninitialised pool or a NULL d_cost.  SVOSLAM_ERR_POOL_LIMIT, decided before anything is allocated or written: more than
 *     2^31 - 1 cells, row words or elements of an intermediate of the region inflated by r horizontally, 1 below and H - 1 above;
 *     more than 2^24 - 1 tiles of 64 x 8 x 8 cells; n_out * (1 + c * S) >= 2^30 (the value of "not reached").  SVOSLAM_ERR_OOM: an
 *     allocation failed; the slots the call grew are released, after the stream has drained.  SVOSLAM_ERR_HIP with a text in
 *     svoslam_last_error: the round cap (tiles * cells per tile + 1) was reached, which the argument of section 23 rules out.
 *
 * svoslam_field_trace_ground_paths (no pool, no workspace)
 *   d_field: any int32 array in device memory laid out as d_cost over the region; -2 = not a foothold, -1 = a foothold that cannot
 *     be reached, >= 0 a cost-to-go.  up, step_cells, climb_cost and snap_cells as above (step_cells 0..SVOSLAM_MAX_STEP_CELLS; no
 *     height is needed).  d_starts: n_starts triples (x, y, z) of int32 absolute cells, in device memory.
 *   Snapping: the foothold of a start is the first cell with a value other than -2, going from the start against u, the start itself
 *     first, within snap_cells further cells, inside the region.  A start outside the region, without a foothold, or whose foothold
 *     holds -1 has length 0 and stores nothing.
 *   The walk begins at the foothold.  From a cell q of value v > 0 it moves to the FIRST candidate q' = q + e + j u inside the region
 *     whose value v' satisfies v' >= 0 and v' + 1 + c |j| == v.  Candidates are ordered by e first -- minus then plus along x, then
 *     minus and plus along the other horizontal axis -- and within one e by j = 0, -1, +1, -2, +2, ... up to |j| = S.  (The smallest
 *     neighbour value alone is not a predecessor here: moves into one cell differ in price.)  The walk ends at value 0.  If no
 *     candidate qualifies it stops, and the length is MINUS the number of cells walked.  The values fall strictly, so the walk is
 *     bounded by its data.
 *   Outputs: d_paths and d_lengths exactly as svoslam_field_trace_paths writes them: the length counts the whole path even beyond
 *     max_cells, nothing behind the stored cells is written.  Asynchronous on `stream`, nothing is read back; one
 *     SVOSLAM_STAGE_QUERY bracket.
 *   Errors: those of svoslam_field_trace_paths, and SVOSLAM_ERR_INVALID_ARG for `up` outside 2..5, step_cells, climb_cost or
 *     snap_cells outside their ranges. */
#define SVOSLAM_MAX_STEP_CELLS 4
#define SVOSLAM_MAX_HEIGHT_CELLS 256
#define SVOSLAM_MAX_SNAP_CELLS 256
typedef struct { int32_t footholds, seeds_used, rounds, tile_runs; } svoslam_ground_stats;
int svoslam_pool_ground_field(svoslam_workspace *ws, const svoslam_pool *pool, int32_t max_depth, const int32_t origin_cell[3],
                              const int32_t dims[3], int32_t up /* 2 +y, 3 -y, 4 +z, 5 -z */, int32_t radius_cells,
                              int32_t height_cells, int32_t step_cells, int32_t climb_cost, int32_t snap_cells, const int32_t *d_seeds,
                              int32_t n_seeds, int32_t *d_cost, svoslam_ground_stats *stats /* may be NULL */, void *stream);
int svoslam_field_trace_ground_paths(const int32_t *d_field, const int32_t origin_cell[3], const int32_t dims[3], int32_t up,
                                     int32_t step_cells, int32_t climb_cost, int32_t snap_cells, const int32_t *d_starts,
                                     int32_t n_starts, int32_t max_cells,
                                     int32_t *d_paths /* [n_starts][max_cells][3], may be NULL if max_cells == 0 */,
                                     int32_t *d_lengths /* [n_starts] */, void *stream);
/* diagnostics: the device pointers and sizes in bytes of the workspace's six ground-field slots (the occupancy bit rows of the
 * inflated region; the planar transform's values after its x pass; after its second pass; the body bit rows D; the foothold bit
 * rows G; the control record with the tile flags; NULL / 0 before the first call that needs them), as
 * svoslam_workspace_plan_buffers shows the cost field's.  Host only. */
int svoslam_workspace_ground_buffers(const svoslam_workspace *ws, void *d_ptrs[6], uint64_t bytes[6]);
/* The library's own sort and scan, exposed for tests and tools (no reference counterpart).  Every map operation sorts Morton keys
 * with the stable LSD radix sort of csrc/radix_sort.hip and compacts with its exclusive scan; these two calls reach them with
 * arguments of the caller's choosing, where the map's calls choose the form and the digit width from n.  All arrays are in device
 * memory; both calls are asynchronous on `stream` and use grow-only slots of the workspace (the sort's ping-pong arrays and
 * histograms, the scan's chunk sums), so the workspace's sort phase outcome (svoslam_svo_fuse_sort, _adopt_sorted) is void after
 * svoslam_sort_words.
 *   svoslam_sort_words sorts n 64-bit words.  Stable: R1, equal keys leave in the order they came in.
 *     idx_bits >= 0, the packed form: a word is key << idx_bits | index.  The words are sorted on their key bits
 *       [idx_bits, idx_bits + key_bits) in passes of digit_bits bits or fewer (1..11; 0: the width the map's calls take for n
 *       elements), tiles of 2048 words.  d_keys_out[i] = word >> idx_bits of the i-th sorted word -- bits above the key included,
 *       which order nothing -- and, if want_vals != 0, d_vals_out[i] = the low 32 bits of word & (2^idx_bits - 1).  d_vals is
 *       ignored.  idx_bits = 0: the keys alone (the voxel-grid form).
 *     idx_bits == -1, the pair form: the words are sorted on bits [0, key_bits) in 8-bit passes, tiles of 1024, carrying a 32-bit
 *       value each: d_vals[i], or i where d_vals is NULL.  d_keys_out = the whole words in sorted order; d_vals_out = the carried
 *       values, if want_vals != 0.  digit_bits is not used.
 *     d_vals_out may be NULL when want_vals == 0.  The outputs may be the inputs.
 *     SVOSLAM_ERR_INVALID_ARG: NULL ws; n < 0; with n > 0 a NULL d_words, d_keys_out, or d_vals_out with want_vals != 0;
 *     key_bits < 1; idx_bits < -1; key_bits + max(idx_bits, 0) > 64; digit_bits outside 0..11.  n == 0 with valid arguments is
 *     SVOSLAM_OK and launches nothing.
 *   svoslam_exclusive_scan_u32 replaces d_data[i] by (d_data[0] + ... + d_data[i - 1]) mod 2^32, in place, and writes the sum of
 *     all n elements mod 2^32 to *d_total (device memory).  n <= 8192 is one workgroup's loop; longer arrays are scanned in chunks
 *     of 2048 on any number of workgroups.  n == 0 writes *d_total = 0 (d_data may then be NULL).  SVOSLAM_ERR_INVALID_ARG: NULL
 *     ws or d_total, NULL d_data with n > 0, n > 2^32 - 2048. */
int svoslam_sort_words(svoslam_workspace *ws, const unsigned long long *d_words, const uint32_t *d_vals, int32_t n, int32_t key_bits,
                       int32_t idx_bits, int32_t digit_bits, int32_t want_vals, unsigned long long *d_keys_out, uint32_t *d_vals_out,
                       void *stream);
int svoslam_exclusive_scan_u32(svoslam_workspace *ws, uint32_t *d_data, uint32_t n, uint32_t *d_total, void *stream);
/* device allocation / copies for callers that do not link the HIP runtime themselves (blocking copies) */
int svoslam_malloc(void **d_ptr, size_t bytes);
int svoslam_memcpy_h2d(void *d_dst, const void *h_src, size_t bytes);
int svoslam_memcpy_d2h(void *h_dst, const void *d_src, size_t bytes);

/* ------------------------------------------------------------------------
 * Mesh path (configs 1, 2, 5): OBJ/BMP loading and mesh -> voxel grid
 * ---------------------------------------------------------------------- */
/* Mesh of include/octree_slam/common_types.h:20-32 as Scene::loadObjFile fills it
 * (src/world/scene.cpp:26-33,115-133): HOST arrays, non-indexed (9 floats per triangle),
 * recentred (x/z centred, y min = 0; obj.cpp:227-238). */
typedef struct {
  float *vbo;       /* 9 * n_tris floats */
  float *tbo;       /* 6 * n_tris floats (uv per vertex) or NULL */
  int32_t n_tris;
  int32_t tbosize;  /* floats in tbo */
  float bbox0[3], bbox1[3];
} svoslam_mesh;
/* bmp_texture of common_types.h:34-38: HOST width*height*3 floats, r,g,b in 0..1 */
typedef struct {
  float *data;
  int32_t width, height;
} svoslam_texture;
/* Scene::loadObjFile (scene.cpp:26-33) = objLoader + obj::buildVBOs + objToMesh */
int svoslam_mesh_load_obj(const char *path, svoslam_mesh *out);
int svoslam_mesh_free(svoslam_mesh *mesh);
/* Scene::loadBMP (scene.cpp:35-62) */
int svoslam_texture_load_bmp(const char *path, svoslam_texture *out);
int svoslam_texture_free(svoslam_texture *tex);
/* replaces voxelization::meshToVoxelGrid (include/octree_slam/world/voxelization/voxelization.h:21,
 * src/world/voxelization/voxelization.cu:381-405) with N = 2^log_N cells per axis over the mesh's own
 * AABB (the reference fixes log_N = 8, log_T = 3: voxelization.cu:24-25).  tex may be NULL (voxels are
 * green, voxelization.cu:101-103).  Outputs are hipMalloc'ed n x vec4 arrays in ascending framebuffer
 * (tiled) index order, free with svoslam_free; d_indices (optional) receives those indices;
 * *scale_out = computeScale (half a voxel edge along x).  Blocking. */
int svoslam_mesh_to_voxel_grid(svoslam_workspace *ws, const svoslam_mesh *mesh, const svoslam_texture *tex, int32_t log_N,
                               int32_t log_T, float **d_centers, float **d_colors, unsigned long long **d_indices,
                               int32_t *n_out, float *scale_out, void *stream);
/* Statistics of the workspace's LAST svoslam_mesh_to_voxel_grid (measurement aid, no reference counterpart): the number of
 * (cell, triangle) fragments the scan-line rasteriser emitted and sorted -- the unit of the voxelizer's per-stage algorithmic
 * bytes; 0 before any call. */
int svoslam_mesh_last_fragments(const svoslam_workspace *ws, int64_t *fragments_out);

/* replaces voxelization::voxelGridToMesh (include/octree_slam/world/voxelization/voxelization.h:19,
 * src/world/voxelization/voxelization.cu:184-217, :325-379; SURVEY 8f.4, a display aid): one copy of the cube mesh
 * (host arrays: cube_vbosize floats of positions and of normals, cube_ibosize indices) per voxel, positions
 * cube * scale_factor + centre, colours replicated per vertex component, indices + idx * cube_ibosize (the
 * reference's offset).  scale_factor = computeScale(bbox) / CUBE_MESH_SCALE (0.1) in the reference.  Outputs are
 * device arrays of the caller: n * cube_vbosize floats (vbo, nbo, cbo), n * cube_ibosize ints (ibo).  Blocking. */
int svoslam_voxel_grid_to_mesh(svoslam_workspace *ws, const float *d_centers, const float *d_colors, int32_t n, float scale_factor,
                               const float *cube_vbo, int32_t cube_vbosize, const int32_t *cube_ibo, int32_t cube_ibosize,
                               const float *cube_nbo, float *d_vbo, int32_t *d_ibo, float *d_nbo, float *d_cbo, void *stream);

/* ------------------------------------------------------------------------
 * Recorded-sensor input: replaces sensor::OpenNIDevice
 * (src/sensor/openni_device.cpp:13-150) as the producer of RawFrame (common_types.h:65-73).
 * The association file is a TUM-RGB-D style list, one frame per line:
 *   <timestamp> <file> <timestamp> <file>     (depth and colour image in either order, '#' comments,
 *   paths relative to the list).  Images: PNG (8-bit RGB, 16-bit grey), binary PGM (16 bit) / PPM.
 * depth_units_per_metre converts the stored depth to the millimetres of RawFrame (1000 = already mm,
 * 5000 = TUM).  Timestamps are returned in microseconds.
 * ---------------------------------------------------------------------- */
typedef struct svoslam_frame_reader svoslam_frame_reader;
int svoslam_frame_reader_open(svoslam_frame_reader **reader, const char *association_file, float depth_units_per_metre);
int svoslam_frame_reader_close(svoslam_frame_reader *reader);
int svoslam_frame_reader_info(const svoslam_frame_reader *reader, int32_t *width, int32_t *height, int32_t *num_frames);
int svoslam_frame_reader_rewind(svoslam_frame_reader *reader);
/* next frame into HOST buffers (width*height uint16 / width*height*3 bytes); *got = 0 at the end of the list */
int svoslam_frame_reader_next_host(svoslam_frame_reader *reader, uint16_t *h_depth, uint8_t *h_color, long long *timestamp,
                                   int32_t *got);
/* OpenNIDevice::readFrame (:93-150): next frame into DEVICE buffers (pinned staging + async upload on `stream`) */
int svoslam_frame_reader_next(svoslam_frame_reader *reader, uint16_t *d_depth, uint8_t *d_color, long long *timestamp,
                              int32_t *got, void *stream);
/* openni_device.cpp:64-65: focal = size / (2 tan(fov / 2)), fov in radians */
int svoslam_focal_from_fov(int32_t width, int32_t height, float hfov_rad, float vfov_rad, float *fx, float *fy);
/* one image file into a malloc'ed host buffer (free with free()); 16-bit samples in host byte order */
int svoslam_image_load(const char *path, void **h_data, int32_t *width, int32_t *height, int32_t *channels, int32_t *bits);

/* ------------------------------------------------------------------------
 * Host objects: world::Scene + world::Octree (include/octree_slam/world/scene.h:20-81,
 * octree.h:80-125; src/world/scene.cpp, octree.cpp:251-385) as an opaque handle.
 * ---------------------------------------------------------------------- */
typedef struct svoslam_scene svoslam_scene;
int svoslam_scene_create(svoslam_scene **scene);                       /* Scene::Scene, scene.cpp:11-17 */
int svoslam_scene_destroy(svoslam_scene *scene);
int svoslam_scene_load_obj(svoslam_scene *scene, const char *path);    /* Scene::loadObjFile, scene.cpp:26-33 */
int svoslam_scene_load_bmp(svoslam_scene *scene, const char *path);    /* Scene::loadBMP, scene.cpp:35-62 */
/* optional: create the Octree explicitly (resolution, root centre, root half edge) before the first
 * insertion and/or pin the tree depth (depth_override > 0) instead of deriving it from
 * ceil(log2(edge/resolution)) (octree.cpp:284).  The reference derives everything from the first
 * cloud / mesh bounding box (scene.cpp:77-79,101). */
int svoslam_scene_set_octree(svoslam_scene *scene, float resolution, const float center[3], float size,
                             int32_t depth_override);
/* Scene::voxelizeMeshes(octree), scene.cpp:64-85.  log_N <= 0 selects the reference's 8. */
int svoslam_scene_voxelize_meshes(svoslam_scene *scene, int32_t octree, int32_t log_N, void *stream);
/* Scene::extractVoxelGridFromOctree, scene.cpp:87-96 (scale 0.01) */
int svoslam_scene_extract_voxel_grid(svoslam_scene *scene, void *stream);
/* Scene::addPointCloudToOctree, scene.cpp:98-113 (bbox = computePointCloudBoundingBox of the cloud) */
int svoslam_scene_add_point_cloud(svoslam_scene *scene, const float origin[3], const float *d_points,
                                  const uint8_t *d_colors, int32_t n, const float bbox0[3], const float bbox1[3],
                                  void *stream);
/* Scene::voxel_grid() accessor: device vec4 arrays owned by the scene */
int svoslam_scene_voxel_grid(svoslam_scene *scene, const float **d_centers, const float **d_colors, int32_t *n,
                             float *scale);
/* Scene::svo(bbox) -> Octree::extractSVO (octree.cpp:339-360): non-owning view of the pool */
int svoslam_scene_svo(svoslam_scene *scene, const uint32_t **d_data, float center[3], float *size, int32_t *num_nodes,
                      int32_t *max_depth);

/* ------------------------------------------------------------------------
 * Rendering
 * ---------------------------------------------------------------------- */
#define SVOSLAM_RENDER_REFERENCE 0 /* pixel stored only on retirement, as the reference does */
#define SVOSLAM_RENDER_CARRY 1     /* local pixel carried across march steps */

/* replaces rendering::coneTraceSVO (include/octree_slam/rendering/
 * cone_tracing_kernels.h:16, src/rendering/cone_tracing_kernels.cu:157-198).
 * d_pos: w*h uchar4 offscreen framebuffer (stands in for the mapped GL PBO of
 * cuda_renderer.cpp:158-171).  view = Camera.view.  d_steps (optional, may be
 * NULL): 2 x uint64 device counters {march steps, levels descended} the kernel
 * adds to (for the bytes model). */
int svoslam_cone_trace_svo(uint8_t *d_pos, int32_t width, int32_t height, float fov, const float view[16],
                           const uint32_t *d_octree, const float center[3], float size, int32_t mode,
                           unsigned long long *d_steps, void *stream);

/* Row band of the same render: traces rows [row_first, row_first+rows) of the
 * width x height frame into the full-frame buffer d_pos (multi-GPU image tiles). */
int svoslam_cone_trace_svo_band(uint8_t *d_pos, int32_t width, int32_t height, int32_t row_first, int32_t rows,
                                float fov, const float view[16], const uint32_t *d_octree, const float center[3],
                                float size, int32_t mode, unsigned long long *d_steps, void *stream);
/* Re-entrancy: the per-render acceleration data (level grid, split-plane tables) lives in a library-owned buffer PER
 * STREAM (17 MB, 135 MB for renders of a megapixel and more): renders enqueued on one stream share it in stream order,
 * renders on different streams never touch each other's; calls may come from several host threads.  The timing log
 * below and svoslam_timer_* are process-wide.  _release frees the buffer of one stream (all_streams != 0: of every
 * stream) once the caller has synchronised it. */
int svoslam_cone_trace_release(void *stream, int32_t all_streams);
/* Measurement aid: while enabled, every cone-trace call brackets its trace kernel (not the small
 * acceleration-structure build before it) with a pair of HIP events on the launch stream.
 * _read waits for the logged launches, returns the summed kernel time and their number, and clears the log. */
int svoslam_cone_trace_timing(int32_t enable);
int svoslam_cone_trace_timing_read(float *h_ms_sum, int32_t *h_launches);
/* The same for every stage of the frame (bench.py's per-stage rooflines; startTiming / stopTiming of
 * src/utils/timing_utils.cu:11-32 applied per stage): bit s of `mask` turns stage s on -- its launches are bracketed by
 * a pair of HIP events on the stream they run on (~2.6 us of that stream per record).  svoslam_stage_timing clears
 * every log; _read waits for the logged pairs of one stage, returns their summed duration and number, clears that log.
 * svoslam_cone_trace_timing(e) == turning SVOSLAM_STAGE_MARCH on / off. */
#define SVOSLAM_STAGE_MARCH 0        /* cone_trace_kernel alone */
#define SVOSLAM_STAGE_TRACKER 1      /* the 19 ICP iterations of a frame (one launch, or the launch chain) */
#define SVOSLAM_STAGE_FUSE_SORT 2    /* keys (+ back-projection in the frame loop) + radix sort */
#define SVOSLAM_STAGE_FUSE_PLAN 3    /* split planning (+ the early tile initialisation) */
#define SVOSLAM_STAGE_FUSE_COMMIT 4  /* splits, leaf blend, mip levels */
#define SVOSLAM_STAGE_MAPS 5         /* bilateral filter + vertex / normal pyramids */
#define SVOSLAM_STAGE_MESH_RASTER 6  /* meshToVoxelGrid: scan-line counts + scans + fragment emission (incl. the two count readbacks) */
#define SVOSLAM_STAGE_MESH_SORT 7    /* meshToVoxelGrid: sort of the (cell, triangle) fragments */
#define SVOSLAM_STAGE_MESH_EMIT 8    /* meshToVoxelGrid: last fragment per cell -> voxel centres + colours (incl. the count readback) */
#define SVOSLAM_STAGE_SURFACE_BFS 9    /* extract_surface_mesh: the occupied cells (incl. one readback per level) */
#define SVOSLAM_STAGE_SURFACE_FACES 10 /* extract_surface_mesh: face masks + scan (incl. the count readback) | emission: two brackets per call, the host's allocations between them are outside */
#define SVOSLAM_STAGE_SURFACE_WELD 11  /* extract_surface_mesh: corner sort + run heads + scan (incl. the count readback) | scatter: two brackets per call likewise */
#define SVOSLAM_STAGE_QUERY 12         /* svoslam_pool_cast_rays / _query_points / _count_boxes / _nearest_occupied: the kernel, one bracket per call; svoslam_pool_distance_field: its four launches, one bracket per call; svoslam_pool_reach_field: the field's launches and every launch and readback of the relaxation, one bracket per call; svoslam_pool_label_components: the field's launches and its own, one bracket per call; svoslam_pool_nearest_field: its five launches, one bracket per call; svoslam_pool_visibility_field: its two launches, one bracket per call; svoslam_score_poses: its one to three launches, one bracket per call; svoslam_pool_cost_field: the field's launches and every launch and readback of the relaxation, one bracket per call; svoslam_field_trace_paths: its launch, one bracket per call; svoslam_pool_cover_views: its launches, the readback of T and all k_max rounds, one bracket per call; svoslam_field_observe_rays: its two clears and two launches, one bracket per call; svoslam_pool_frontier_field: its clear and two launches, one bracket per call */
#define SVOSLAM_STAGE_COUNT 13
int svoslam_stage_timing(uint32_t mask);
int svoslam_stage_timing_read(int32_t stage, float *h_ms_sum, int32_t *h_pairs);

/* ------------------------------------------------------------------------
 * Sensor image kernels (include/octree_slam/sensor/image_kernels.h:21-55,
 * src/sensor/image_kernels.cu)
 * ---------------------------------------------------------------------- */
/* generateVertexMap, image_kernels.h:24 / .cu:24-58 */
int svoslam_generate_vertex_map(const uint16_t *d_depth, float *d_vertex, int32_t width, int32_t height, float fx,
                                float fy, int32_t img_w, int32_t img_h, void *stream);
/* same, restricted to image rows [first_row, first_row+rows) of the full-frame buffers
 * (row band of a multi-GPU image split); pixel coordinates stay absolute */
int svoslam_generate_vertex_map_rows(const uint16_t *d_depth, float *d_vertex, int32_t width, int32_t height,
                                     int32_t first_row, int32_t rows, float fx, float fy, int32_t img_w, int32_t img_h,
                                     void *stream);
/* generateNormalMap, image_kernels.h:30 / .cu:104-139 */
int svoslam_generate_normal_map(const float *d_vertex, float *d_normal, int32_t width, int32_t height, void *stream);
/* bilateralFilter, image_kernels.h:34 / .cu:142-186 */
int svoslam_bilateral_filter(const uint16_t *d_in, uint16_t *d_out, int32_t width, int32_t height, void *stream);
/* subsampleDepth<uint16_t|float>, image_kernels.h:41-42 / .cu:236-289.  In place:
 * the (width/2 x height/2) result overwrites the head of d_data. d_tmp: scratch of
 * width*height/4 elements (the reference cudaMallocs it per call). */
int svoslam_subsample_depth_u16(uint16_t *d_data, uint16_t *d_tmp, int32_t width, int32_t height, void *stream);
int svoslam_subsample_depth_f32(float *d_data, float *d_tmp, int32_t width, int32_t height, void *stream);
/* subsample<float|Color256>, image_kernels.h:37-38 / .cu:291-326 */
int svoslam_subsample_f32(float *d_data, float *d_tmp, int32_t width, int32_t height, void *stream);
int svoslam_subsample_rgb8(uint8_t *d_data, uint8_t *d_tmp, int32_t width, int32_t height, void *stream);
/* colorToIntensity, image_kernels.h:45 / .cu:188-203 */
int svoslam_color_to_intensity(const uint8_t *d_rgb, float *d_out, int32_t n, void *stream);
/* transformVertexMap / transformNormalMap, image_kernels.h:52,55 / .cu:206-234 */
int svoslam_transform_vertex_map(float *d_vertex, const float trans[16], int32_t n, void *stream);
int svoslam_transform_normal_map(float *d_normal, const float trans[16], int32_t n, void *stream);
/* computePointCloudBoundingBox, image_kernels.h:27 / .cu:60-102.  bbox0/bbox1 are
 * host in/out (zero = unset sentinel).  Blocking. */
int svoslam_point_cloud_bbox(const float *d_points, int32_t n, float h_bbox0[3], float h_bbox1[3], void *stream);
/* non-blocking form for a device-resident frame loop: d_out7 = {min x,y,z, max x,y,z,
 * any_valid} of the valid points (no "zero = unset" merge with a previous box) */
int svoslam_point_cloud_bbox_device(svoslam_workspace *ws, const float *d_points, int32_t n, float *d_out7,
                                    void *stream);

/* ------------------------------------------------------------------------
 * ICP (include/octree_slam/sensor/localization_kernels.h:17-42,
 * src/sensor/localization_kernels.cu)
 * ---------------------------------------------------------------------- */
/* Photometric RGB-D term.  The reference DECLARES gradient / difference (image_kernels.h:45-49) and
 * computeRGBDCost (localization_kernels.h:42) but ships no definition of the first two, an empty body for the third
 * (localization_kernels.cu:328-331) and its call site commented out (rgbd_camera.cpp:126-141; W_RGBD = 0.1, :20).
 * There is no reference behaviour to match; the specification is this build's own (restated in
 * oracle/svoslam_oracle.c):
 *   gradient    Sobel 3x3 / 8 on interior pixels, (0,0) on the border; d_gradient = (gx, gy) per pixel
 *   difference  out = in1 - in2
 *   rgbd_cost   same-index association as computeICPCost2 (no reprojection), gates = finite + depth range + distance;
 *               r = I_last - I_cur; J = G_T * (gx du/dv + gy dv/dv) with the LAST frame's gradient, the pinhole
 *               derivative at the CURRENT vertex and the geometric term's own G_T rows (:208-213), so that both systems
 *               share one parametrisation; exact fixed-point sums.  fx, fy and the full image size are extra
 *               parameters (the reference's RGBDFrame carries no intrinsics).  Blocking (h_A, h_b on the host).
 *   svoslam_camera_set_rgbd(cam, 1), before the first frame: every ICP iteration solves A1 + W_RGBD A2, b1 + W_RGBD b2
 *   (the commented-out block of rgbd_camera.cpp:130-141); default off = the reference as shipped. */
int svoslam_gradient(const float *d_intensity, float *d_gradient, int32_t width, int32_t height, void *stream);
int svoslam_difference(const float *d_in1, const float *d_in2, float *d_out, int32_t n, void *stream);
int svoslam_rgbd_cost(const float *d_last_intensity, const float *d_last_gradient, const float *d_last_vertex,
                      const float *d_cur_intensity, const float *d_cur_vertex, int32_t width, int32_t height, float fx, float fy,
                      int32_t img_width, int32_t img_height, float h_A[36], float h_b[6], void *stream);
/* computeICPCost2, localization_kernels.h:39 / .cu:154-229,303-326.  h_A (36) and
 * h_b (6) are host outputs as in the reference.  Blocking. */
int svoslam_icp_cost2(const float *d_last_vertex, const float *d_last_normal, const float *d_cur_vertex,
                      const float *d_cur_normal, int32_t width, int32_t height, float h_A[36], float h_b[6],
                      void *stream);
/* computeICPCost, localization_kernels.h:38 / .cu:59-152,231-301: the variant with an explicit
 * correspondence stencil (finite, distance and normal gates; no depth-range gate), load size 10 and a
 * reduce over floor(M/10) partials: the first floor(M/10)*10 correspondences in pixel order contribute.
 * With M = 0 h_A and h_b are left untouched, as in the reference (:251-253).  *num_correspondences
 * (may be NULL) receives M.  Blocking. */
int svoslam_icp_cost(const float *d_last_vertex, const float *d_last_normal, const float *d_cur_vertex,
                     const float *d_cur_normal, int32_t width, int32_t height, float h_A[36], float h_b[6],
                     int32_t *num_correspondences, void *stream);
/* Non-blocking building block used by the tracker and by multi-GPU row bands:
 * adds the 27 exact fixed-point accumulators (21 upper-triangle A terms then 6
 * b terms, carried in float64) of pixels [first_pixel, first_pixel+num_pixels)
 * into d_acc[27].  Integer-valued doubles: sums are exact and associative, so
 * band partials can be all-reduced (RCCL sum, float64) in any order. */
int svoslam_icp_accumulate(const float *d_last_vertex, const float *d_last_normal, const float *d_cur_vertex,
                           const float *d_cur_normal, int32_t width, int32_t height, int32_t first_pixel,
                           int32_t num_pixels, double *d_acc, void *stream);

/* ------------------------------------------------------------------------
 * Tracker: host mirror of sensor::RGBDCamera (include/octree_slam/sensor/
 * rgbd_camera.h, src/sensor/rgbd_camera.cpp) with every per-iteration step
 * (accumulate, 6x6 Cholesky, pose compose) resident on the device.
 * ---------------------------------------------------------------------- */
typedef struct svoslam_camera svoslam_camera;
/* RGBDCamera::RGBDCamera, rgbd_camera.cpp:22-24.  band_first_row/band_rows select
 * the image rows this process owns for ICP accumulation (0, height = all). */
int svoslam_camera_create(svoslam_camera **cam, int32_t width, int32_t height, float fx, float fy);
int svoslam_camera_destroy(svoslam_camera *cam);
/* back to a new RGBDCamera (identity pose, no frame seen) keeping its buffers.  Blocking. */
int svoslam_camera_reset(svoslam_camera *cam);
int svoslam_camera_set_band(svoslam_camera *cam, int32_t first_row, int32_t rows);
/* RGBDCamera::update, rgbd_camera.cpp:53-191.  Non-blocking.  Returns 1 in
 * *processed if the frame was used, 0 if its timestamp was stale (:55-59). */
int svoslam_camera_update(svoslam_camera *cam, const uint16_t *d_depth, const uint8_t *d_rgb, long long timestamp,
                          int32_t *processed, void *stream);
/* update() in its two halves, for callers that overlap them: prepare() filters the depth image and builds
 * the vertex/normal pyramids of the next frame (independent of earlier poses; up to two frames may be
 * prepared ahead), track() estimates the pose of the oldest prepared frame.  update() == prepare() then
 * track() on one stream.  With several streams the caller orders prepare(f) after track(f-2) and
 * track(f) after prepare(f) (the maps live in three rotating sets). */
int svoslam_camera_prepare(svoslam_camera *cam, const uint16_t *d_depth, const uint8_t *d_rgb, long long timestamp,
                           int32_t *processed, void *stream);
int svoslam_camera_track(svoslam_camera *cam, void *stream);
/* Frame-parallel tracking (several GPUs, or several streams of one).  RGBDCamera::update starts update_trans at the
 * identity for every frame (rgbd_camera.cpp:100) and iterates on the maps of frames k-1 and k only (:103-168): a frame's
 * ICP is a function of two depth images; only :172-173 (position, orientation *= update_trans) chain the frames.
 *   pair_delta()  runs :62-168 for the pair (prev, cur) and writes SVOSLAM_DELTA_FLOATS floats to d_delta: update_trans
 *                 (mat4, column-major), the number of pyramid levels abandoned (:148-151) as int32 bits, 3 x padding.
 *                 `cam` serves as scratch (map sets, tracker); its pose afterwards means nothing and it must not be fed by
 *                 update() / apply_delta().  Non-blocking.
 *   apply_delta() :172-173 + main.cpp:40 for a delta from anywhere: a stream of apply_delta(pair_delta(k-1, k)) leaves the
 *                 camera exactly where a stream of update(k) leaves it.  d_delta = NULL, or the camera's first frame (no
 *                 ICP: `pass >= 1`, :99): pose unchanged.  A camera is fed either by update() or by apply_delta(), not both
 *                 (reset in between).  *processed as for update().  Non-blocking. */
#define SVOSLAM_DELTA_FLOATS 20
int svoslam_camera_pair_delta(svoslam_camera *cam, const uint16_t *d_depth_prev, const uint8_t *d_rgb_prev, const uint16_t *d_depth_cur,
                              const uint8_t *d_rgb_cur, float *d_delta, void *stream);
int svoslam_camera_apply_delta(svoslam_camera *cam, const float *d_delta, long long timestamp, int32_t *processed, void *stream);
/* Multi-GPU stepping: update() split at the all-reduce points.  begin() builds
 * the pyramids; for level = 2,1,0 and it = 0..iters(level)-1 call
 * icp_accumulate() [adds this band's 27 doubles into svoslam_camera_acc()], then
 * all-reduce that buffer across ranks, then icp_solve(); finally end(). */
int svoslam_camera_begin(svoslam_camera *cam, const uint16_t *d_depth, const uint8_t *d_rgb, long long timestamp,
                         int32_t *processed, void *stream);
int svoslam_camera_icp_iters(int32_t level); /* PYRAMID_ITERS, rgbd_camera.cpp:19 */
int svoslam_camera_icp_accumulate(svoslam_camera *cam, int32_t level, int32_t iter, void *stream);
double *svoslam_camera_acc(svoslam_camera *cam); /* device double[27] */
/* redirect the accumulators to caller-owned device memory (e.g. a torch tensor that
 * torch.distributed all-reduces); NULL restores the internal buffer.  Must be zeroed
 * by the caller once; icp_solve() re-zeroes it after every iteration. */
int svoslam_camera_set_acc(svoslam_camera *cam, double *d_acc);
/* number of pyramid levels abandoned because the solve returned NaN
 * ("Camera tracking is lost.", rgbd_camera.cpp:148-151).  Blocking. */
int svoslam_camera_tracking_lost_count(svoslam_camera *cam, int32_t *count, void *stream);
/* switches the photometric RGB-D term on (see svoslam_rgbd_cost above); only before the first frame */
int svoslam_camera_set_rgbd(svoslam_camera *cam, int32_t enable);
/* strict = 1 (default): RGBDCamera::update as the reference has it, every quirk included.  strict = 0: this build's CORRECTED
 * tracker (own specification, no reference behaviour; SURVEY section 7 step 1 "every Appendix-B quirk behind a strict_reference
 * switch").  Three places where the reference's update is not a rigid-motion estimate are replaced, everything else -- gates,
 * pyramid, iteration counts, exact fixed-point sums, Cholesky, glm products -- stays:
 *   - the rotational rows of the Jacobian are those of [v2]x (A_T[0..2] = v2 x n1) instead of the rows of
 *     src/sensor/localization_kernels.cu:207-213 (Q14);
 *   - this_trans = translate(x3, x4, x5) * Rz(x2) * Ry(x1) * Rx(x0) (a current-frame point goes to R v + t) instead of
 *     Rz(-x2) * Ry(-x1) * Rx(-x0) * translate(..) (rgbd_camera.cpp:154-158);
 *   - position = (position + t) * update_trans in the row-vector product of rgbd_camera.cpp:172 (Q17 drops t), so that
 *     main.cpp:40's orientation * (x + position) composes the frame-to-frame transforms.
 * Restated in oracle/svoslam_oracle.c (ora_camera_set_strict_reference) and a second time in tests/test_oracle_second_opinion.py
 * (track_second_opinion(..., corrected=True)).
 * Before the first frame only; not combined with the photometric term. */
int svoslam_camera_set_strict_reference(svoslam_camera *cam, int32_t strict);
/* Frame-to-model tracking (second half).  OWN SPECIFICATION: the reference tracks every frame against the
 * previous FRAME's maps and leaves the rest as a TODO (src/sensor/rgbd_camera.cpp:185: "ICP should not swap, as
 * last_frame should be updated by a different function"); these three entry points are that different function.
 *   svoslam_raycast_model_depth   the map ray-cast into a depth image in the SENSOR's pixel grid and unit: pixel (x, y)
 *       looks along ((x - w/2)/fx, (h/2 - y)/fy, 1) (the direction generateVertexMap gives it, image_kernels.cu:24-58)
 *       carried into the map by cam_to_world (the fusion transform of main.cpp:40; exactly one of the host matrix /
 *       the device pointer -- e.g. svoslam_camera_fusion_transform_device -- is given); marched as coneTrace marches
 *       (cone_tracing_kernels.cu:53-146, pixel scale 1/fy) to the first sample whose node has A >= 254; the pixel is
 *       rint(1000 z) as uint16, 0 = nothing met.  d_steps (optional): 1 x uint64 device counter of march steps.
 *   svoslam_camera_set_model_depth   such an image goes through the front end of a sensor frame (bilateral filter,
 *       pyramid, vertex + normal maps: rgbd_camera.cpp:62-93) into a map set of its own.  Non-blocking, stream-ordered.
 *       d_depth == NULL: no model -- the following frames are tracked against the previous frame, until the next one.
 *   svoslam_camera_set_frame_to_model(cam, 1)   every ICP iteration associates the incoming frame with that set (once one
 *       has been given) instead of the previous frame's maps; everything else -- gates, sums, solve, pose composition
 *       -- is RGBDCamera::update unchanged.  Not combined with the photometric term (SVOSLAM_ERR_INVALID_ARG).
 * Restated on the CPU as ora_raycast_model_depth / ora_camera_set_model_depth / ora_camera_set_frame_to_model. */
int svoslam_raycast_model_depth(uint16_t *d_depth, int32_t width, int32_t height, float fx, float fy, const float *cam_to_world,
                                const float *d_cam_to_world, const uint32_t *d_octree, const float center[3], float size,
                                unsigned long long *d_steps, void *stream);
int svoslam_camera_set_model_depth(svoslam_camera *cam, const uint16_t *d_depth, void *stream);
int svoslam_camera_set_frame_to_model(svoslam_camera *cam, int32_t enable);
/* the newest timestamp the camera has accepted (rgbd_camera.cpp:55-59 skips frames that are not newer); *have = 0
 * before the first frame.  Host state, no device access. */
int svoslam_camera_latest_timestamp(svoslam_camera *cam, int32_t *have, long long *timestamp);
/* plan of the most recent tracked frame: out[0] form (0 no ICP yet, 1 launch chain, 2 one launch register form
 * (variant 0), 3 one launch streaming form (variant 1), 4 hybrid: level 2 in the one launch, levels 1..0 by the chain),
 * out[1] workers, out[2..4] participants[0..2], out[5..7] slots[0..2]; for forms 0 and 1 the last seven are 0, for form 4
 * the entries of levels 1 and 0 are.  Which form a frame takes follows from image size, svoslam_config.track_mode /
 * track_stream / track_workers and the CUs the stream may use.  Host state (what svoslam_camera_track enqueued), no device
 * access; svoslam_camera_reset returns it to form 0.  Frames fed by the stepping API or by apply_delta() do not change it. */
int svoslam_camera_last_track_plan(const svoslam_camera *cam, int32_t out[8]);
/* diagnostic (libraries built with -DSVO_TRK_PROF; zeros otherwise): device clock stamps of the last tracked frame's
 * one-launch tracker, h_stamps[32][8] = per ICP iteration {solver: start, fan-in done, rows summed, published;
 * worker 0: start, terms done, row stored, broadcast received}.  Blocking. */
int svoslam_camera_track_profile(svoslam_camera *cam, unsigned long long *h_stamps, void *stream);
int svoslam_camera_icp_solve(svoslam_camera *cam, int32_t level, int32_t iter, void *stream);
int svoslam_camera_end(svoslam_camera *cam, void *stream);
/* position() / orientation() accessors, rgbd_camera.h:33-36.  Blocking (D2H). */
int svoslam_camera_pose(svoslam_camera *cam, float h_position[3], float h_orientation[9], void *stream);
/* device mat4 = mat4(orientation) * translate(I, position) (main.cpp:40); stays on the device */
const float *svoslam_camera_fusion_transform_device(svoslam_camera *cam);
/* last A, b, x (host copies; blocking) for tests */
int svoslam_camera_last_system(svoslam_camera *cam, float h_A[36], float h_b[6], float h_x[6], void *stream);
/* current-frame pyramid maps (device, level 0..2) for tests: after update() the
 * frames have been swapped, so these are the maps of the frame just processed */
const float *svoslam_camera_last_vertex(svoslam_camera *cam, int32_t level);
const float *svoslam_camera_last_normal(svoslam_camera *cam, int32_t level);

/* transformVertexMap with a DEVICE matrix (keeps main.cpp:40 off the host) */
int svoslam_transform_vertex_map_dmat(float *d_vertex, const float *d_trans, int32_t n, void *stream);

/* ------------------------------------------------------------------------
 * Native frame scheduler: the per-frame loop of main.cpp:31-84 (RGBDCamera::update -> generateVertexMap ->
 * transformVertexMap -> computePointCloudBoundingBox -> Scene::addPointCloudToOctree -> coneTraceSVO), software-
 * pipelined over four HIP streams inside the library (csrc/runner.hip) so that a frame costs the host ~0.1 ms
 * instead of the 0.45 ms of a scripted loop.  Results are those of calling the stages one after the other.
 * svoslam_runner_run enqueues n device-resident frames (depth u16 mm, RGB888; strictly increasing timestamps;
 * views = n column-major 4x4 view matrices) after the work already queued on caller_stream, makes caller_stream
 * wait for all of it, and returns without waiting; d_image receives rows [row_first, row_first + rows) of each
 * frame's raycast (the last frame's remain), d_steps (optional) 2 x u64 step / level counters.
 * ---------------------------------------------------------------------- */
typedef struct svoslam_runner svoslam_runner;
int svoslam_runner_create(svoslam_runner **runner, svoslam_camera *cam, svoslam_pool *pool, int32_t width, int32_t height,
                          int32_t max_depth, const float center[3], float edge_length, float fx, float fy, int32_t render_mode);
int svoslam_runner_destroy(svoslam_runner *runner);
/* diagnostic (runner created with SVOSLAM_RUNNER_TIMELINE=1 in the environment): HIP-event times in ms of the stage
 * boundaries of the last call, relative to its first mark: h_ms[frame][10] = {maps begin, maps end, track begin, pose,
 * prepare begin, plan begin, plan end, commit begin, commit end, march end}.  Blocking. */
int svoslam_runner_timeline(svoslam_runner *runner, float *h_ms, int32_t max_frames, int32_t *frames);
int svoslam_runner_run(svoslam_runner *runner, const uint16_t *const *d_depths, const uint8_t *const *d_rgbs,
                       const long long *timestamps, const float *views, int32_t n, uint8_t *d_image, int32_t row_first,
                       int32_t rows, unsigned long long *d_steps, void *caller_stream);
/* The loop with FRAME-TO-MODEL tracking (own specification, see svoslam_raycast_model_depth below: the reference
 * leaves it as a TODO, src/sensor/rgbd_camera.cpp:185).  Per frame: track (against the model set once one has been accepted) ->
 * back-project + fuse -> the map ray-cast into a depth image from the pose just tracked -> accepted as the next frame's model if
 * at least min_coverage (0..1) of its pixels met the map, else the next frame is tracked against the previous frame's maps ->
 * cone-traced view (rows of the LAST frame in d_image).  Sequential on caller_stream and BLOCKING (one 4-byte coverage readback
 * per frame); *models_used (optional) = frames whose model was accepted.  Same call rules as svoslam_runner_run (one caller stream
 * per runner, timestamps newer than the camera's latest).  Leaves frame-to-model tracking switched on in the camera and the last
 * accepted model set, so that a second call continues the sequence as one longer call would; a later svoslam_runner_run on the
 * same runner -- the loop without a model refresh -- clears both when it starts and tracks frame to frame. */
int svoslam_runner_run_model(svoslam_runner *runner, const uint16_t *const *d_depths, const uint8_t *const *d_rgbs,
                             const long long *timestamps, const float *views, int32_t n, uint8_t *d_image, int32_t row_first,
                             int32_t rows, unsigned long long *d_steps, float min_coverage, int32_t *models_used, void *caller_stream);
/* the bounding box the loop computed for the last frame enqueued (computePointCloudBoundingBox, main.cpp:43):
 * {min xyz, max xyz, any point}.  Blocking. */
int svoslam_runner_bbox(svoslam_runner *runner, float h_bbox7[7]);
/* The same loop for ONE RANK of a frame-sharded session (frames are tracked in parallel, one process
 * per GPU, each with a full replica of the map).  The poses come from svoslam_camera_apply_delta(d_deltas[i]) -- n device
 * pointers to SVOSLAM_DELTA_FLOATS floats, produced by svoslam_camera_pair_delta on whichever rank tracked frame i and
 * all-gathered; delta_events (optional; n hipEvent_t, NULL entries allowed): what the pose stream waits for before it reads
 * d_deltas[i] -- so the runner's camera never sees a depth image; EVERY frame is back-projected, planned and committed
 * (the replicas stay byte-identical), and only the frames with march[i] != 0 (march = NULL: all) are ray-marched, frame i
 * into d_images[i].  Entry 0 of d_deltas is ignored for a camera's first frame.  Needs the direct-commit schedule (not an
 * explicit runner_deferred = 1). */
int svoslam_runner_run_sharded(svoslam_runner *runner, const uint16_t *const *d_depths, const uint8_t *const *d_rgbs,
                               const long long *timestamps, const float *views, int32_t n, const float *const *d_deltas,
                               void *const *delta_events, const uint8_t *march, uint8_t *const *d_images, int32_t row_first,
                               int32_t rows, unsigned long long *d_steps, void *caller_stream);
/* The same with the SORT sharded as well (round 3): the rank that owns frame i has back-projected and sorted it
 * (svoslam_svo_fuse_sort_frame with the pose its own chain of svoslam_camera_apply_delta gives, svoslam_svo_fuse_export_sorted)
 * and the sorted arrays have been all-gathered: d_sorted_keys[i] / d_sorted_idx[i] (all n entries required),
 * sorted_events[i] (optional) = what the plan waits for before it reads them.  This rank then only plans and commits every
 * frame and ray-marches its own; the bounding box of svoslam_runner_bbox is not computed in this form. */
int svoslam_runner_run_sharded_presorted(svoslam_runner *runner, const uint16_t *const *d_depths, const uint8_t *const *d_rgbs,
                                         const long long *timestamps, const float *views, int32_t n, const float *const *d_deltas,
                                         void *const *delta_events, const uint8_t *march, uint8_t *const *d_images,
                                         const unsigned long long *const *d_sorted_keys, const uint32_t *const *d_sorted_idx,
                                         void *const *sorted_events, int32_t row_first, int32_t rows, unsigned long long *d_steps,
                                         void *caller_stream);

/* ------------------------------------------------------------------------
 * Timing hook: replaces startTiming/stopTiming (include/octree_slam/
 * timing_utils.h:5-10, src/timing_utils.cu:11-32) with hipEvents on `stream`.
 * ---------------------------------------------------------------------- */
int svoslam_timer_start(void *stream);
int svoslam_timer_stop(void *stream, float *h_ms); /* blocking */

/* ------------------------------------------------------------------------
 * One-shot peer-to-peer exchange of small records between the ranks of one node (csrc/mailbox.hip; SURVEY 5 "comm
 * backend" / 8e).  Replaces the per-iteration 168-byte device-to-host copy of the reference's ICP reduction
 * (src/sensor/localization_kernels.cu:318-325) across GPUs: every rank stores its record into each peer's inbox (device
 * memory mapped by the peers: hipIpc handles between processes, plain pointers inside one) and polls its own; sums are
 * formed in rank order, so every rank gets the same bits.  Two short launches on the caller's stream per collective, no
 * host round trip, no communication library.  All ranks must issue the collectives of a mailbox in the same order.
 * ---------------------------------------------------------------------- */
typedef struct svoslam_mailbox svoslam_mailbox;
int svoslam_mailbox_create(svoslam_mailbox **mailbox, int32_t rank, int32_t world);
int svoslam_mailbox_destroy(svoslam_mailbox *mailbox);
int svoslam_mailbox_handle(svoslam_mailbox *mailbox, void *handle64);                 /* 64 bytes for the other processes */
int svoslam_mailbox_connect(svoslam_mailbox *mailbox, const void *handles);           /* world x 64 bytes, any order of arrival */
int svoslam_mailbox_connect_local(svoslam_mailbox *mailbox, svoslam_mailbox *const *all);  /* peers inside this process */
int svoslam_mailbox_all_gather(svoslam_mailbox *mailbox, const void *d_src, int32_t bytes, void *d_dst, void *stream);
int svoslam_mailbox_all_reduce_f64(svoslam_mailbox *mailbox, double *d_values, int32_t count, void *stream);
/* the two halves of a collective, for callers that drive several mailboxes from one stream (post them all, then collect):
 * _post stages d_src and stores it into every inbox (next epoch), _collect waits for every rank's record of that epoch */
int svoslam_mailbox_post(svoslam_mailbox *mailbox, const void *d_src, int32_t bytes, void *stream);
int svoslam_mailbox_collect(svoslam_mailbox *mailbox, void *d_dst, int32_t bytes, int32_t reduce_f64, void *stream);
int svoslam_mailbox_failed(svoslam_mailbox *mailbox, int32_t *failed);
/* polls per granule before a wait gives up (default 2^24, about a second).  A wait that gives up writes all-ones granules (NaN
 * as binary32 / binary64) in place of the missing record and sets the sticky flag svoslam_mailbox_failed() reports. */
int svoslam_mailbox_set_wait_limit(svoslam_mailbox *mailbox, uint32_t polls);

#ifdef __cplusplus
}
#endif
#endif /* SVOSLAM_H_ */
