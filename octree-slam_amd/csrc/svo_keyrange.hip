// svo_keyrange.hip -- the fusion of one frame cut across ranks by key range (opt-in).  Plan and commit are the
// kernels and the host driver of svo_build.hip, run on the rank's slice of the sorted keys (commit_impl with n_live).
#include "pool_grid.hpp"
#include "pool_state.hpp"
#include "svo_build.hpp"
#include "svo_fuse_internal.hpp"
#include "wave_rank.hpp"

namespace svoslam {

// ----------------------------------------------------------------------------
// key-range sharded commit (protocol pinned on the CPU by tests/test_keyrange_gloo.py)
// ----------------------------------------------------------------------------
// The plan + commit of ONE frame cut across `world` ranks by key range instead of being replicated on every rank.  Every rank holds a
// byte-identical replica of the pool and the frame's sorted keys (sorted by their owners and all-gathered: svo_fuse_export_sorted /
// svo_fuse_merge_sorted).  Two calls per frame and rank, ONE all-gather between them:
//   svo_fuse_keyrange_commit  the rank's slice of the sorted keys -- the keys under a contiguous run of level-3 prefixes holding about
//                             n / world keys (keyrange_bounds_kernel: every rank computes the same cuts) -- is planned (svo.cu:179-237)
//                             and committed (:239-465) by the unchanged kernels as a DEFERRED commit: new tiles beyond the pool's size
//                             in the rank's own numbering, colour words in the shadow array, nothing a replica could not still
//                             discard.  keyrange_pack_* then writes the rank's DELTA: its (pass, depth) bucket sizes, its new tiles
//                             (16 words each, links still in local numbering), the frontier nodes its pass-0 records link from,
//                             {node, colour word} of every existing node it changed, the bricks whose siblings its splits created;
//   [all-gather of the deltas -- the caller's: RCCL, or a table of precomputed deltas for an emulated rank]
//   svo_fuse_keyrange_apply   numbering: the reference numbers the new tiles of a pass by the rank of their key among the pass's sorted
//                             unique keys = bucket-major, key order inside a bucket; slices are key ranges, so rank s's records of
//                             bucket b follow those of ranks < s: global index = bucket base + sum of the lower ranks' counts + local
//                             rank in the bucket -- one table of world x 256 offsets (keyrange_setup_kernel).  Every delta (the own one
//                             included) is written to its global place; the marks of the ray march's grid / bricks are made from ALL the
//                             frame's keys against this replica's own dirty state (ranks render different frames: their dirty states
//                             differ); the colour words of the nodes above the splitter level -- shared by several ranks' paths -- are
//                             recomputed from the merged children, level by level, then the root pass (Q6); size and size readback.
// Frames whose splits reach ABOVE the splitter level (a node of level 1 or 2 without children: the first frames of a map, new territory)
// make several ranks plan the SAME records (the prefix of such a record lies on paths of more than one slice) and create the same tiles:
// every delta lists its records above the splitter level by key, keyrange_setup_kernel ranks them in the ranks' UNION (the reference's
// order inside their buckets) and clears their tiles, and the apply writes of such a tile only the nodes a rank actually filled -- a
// level-3 node has one owner; the shallower ones get the same link from everybody and their colour words from the recomputation.
constexpr int kKrLevel = 3;
constexpr int kKrMaxWorld = 16;
constexpr int kKrHeader = 512;       // words: scalars, then the 256 bucket sizes at [256, 512)
constexpr int kKrSibCap = 8192;      // entries
constexpr int kKrShallowCap = 1024;  // keys (two words each)
constexpr int kKrTopCap = 128;       // records above the splitter level: {key (two words), local record, bucket}; a rank has at most 8 + 64
constexpr int kKrTop0 = kKrHeader + kKrSibCap + 2 * kKrShallowCap;
constexpr int kKrTiles0 = kKrTop0 + 4 * kKrTopCap;  // first word of the tiles
enum { kKrMagic = 0, kKrRecords = 1, kKrWords = 2, kKrLinks = 3, kKrSib = 4, kKrShallow = 5, kKrAnyValid = 6, kKrOverflow = 7, kKrSliceKeys = 8,
       kKrN0 = 9, kKrUsed = 10, kKrCapacity = 11, kKrDepth = 12, kKrTop = 13 };
enum { kKrOverflowed = 2, kKrMismatch = 4 };
constexpr u32 kKrEmpty1 = 127u << 24;  // word1 of a node splitNodes has just created (svo.cu:269-275)
__host__ __device__ inline size_t kr_bid0(u32 records) { return (size_t)kKrTiles0 + 16 * (size_t)records; }
__host__ __device__ inline size_t kr_links0(u32 records) { return kr_bid0(records) + (records + 3u) / 4u; }
__host__ __device__ inline size_t kr_words0(u32 records, u32 links) { return kr_links0(records) + links; }

// window of rank `rank`: win[0] = first, win[1] = end, win[2] = length of its slice of the sorted keys (invalid keys -- key 1 -- sort first
// and belong to nobody).  Cut r lies at the end of the level-L run that holds key number r x valid / world.
__global__ void keyrange_bounds_kernel(const u64 *__restrict__ skey, int n, int depth, int rank, int world, int *__restrict__ win) {
  const int r = (int)threadIdx.x;
  auto first_at_least = [&](int lo, int hi, u64 bound, int shift) {  // first j in [lo, hi) with (skey[j] >> shift) >= bound
    while (lo < hi) { const int mid = (lo + hi) >> 1; if ((skey[mid] >> shift) < bound) lo = mid + 1; else hi = mid; }
    return lo;
  };
  const int v0 = first_at_least(0, n, 2ull, 0);
  const long long nv = n - v0;
  int b = v0;
  if (r >= world) b = n;
  else if (r > 0) {
    const int i = v0 + (int)((long long)r * nv / world);
    if (i > v0) { const int sh = 3 * (depth - kKrLevel); b = first_at_least(i, n, (skey[i - 1] >> sh) + 1ull, sh); }
  }
  if (r <= world) win[4 + r] = b;
  __syncthreads();
  if (r == 0) { const int lo = win[4 + rank], hi = win[4 + rank + 1]; win[0] = lo; win[1] = hi; win[2] = hi - lo; }
}

__global__ __launch_bounds__(256) void keyrange_slice_kernel(const u64 *__restrict__ skey, const u32 *__restrict__ sidx, int n,
                                                             const int *__restrict__ win, u64 *__restrict__ out_key, u32 *__restrict__ out_idx) {
  const int j = (int)(blockIdx.x * 256u + threadIdx.x);
  if (j >= n) return;
  const int lo = win[0], len = win[2];
  out_key[j] = j < len ? skey[lo + j] : 1ull;  // the slice at the front, padding (invalid keys) behind it
  out_idx[j] = j < len ? sidx[lo + j] : 0u;
}

__global__ __launch_bounds__(256) void keyrange_pack_header_kernel(u32 *__restrict__ delta, long long capacity_words, const u32 *__restrict__ bucket_base,
                                                                   const PlanCounts *__restrict__ counts, const u32 *__restrict__ n0_saved,
                                                                   const int *__restrict__ win, int depth) {
  const int t = (int)threadIdx.x;
  delta[256 + t] = bucket_base[t + 1] - bucket_base[t];
  if (t == 0) {
    const u32 R = (u32)counts->total_records, links = (u32)(counts->pass_start[1] - counts->pass_start[0]);
    delta[kKrMagic] = 0x4B52414Eu;
    delta[kKrRecords] = R; delta[kKrWords] = 0u; delta[kKrLinks] = links; delta[kKrSib] = 0u; delta[kKrShallow] = 0u; delta[kKrTop] = 0u;
    delta[kKrAnyValid] = (u32)counts->any_valid; delta[kKrSliceKeys] = (u32)win[2]; delta[kKrN0] = *n0_saved; delta[kKrDepth] = (u32)depth;
    delta[kKrCapacity] = capacity_words > 0xFFFFFFFFll ? 0xFFFFFFFFu : (u32)capacity_words;
    const bool fits = (long long)kr_words0(R, links) <= capacity_words;
    delta[kKrOverflow] = fits ? 0u : 1u;
    delta[kKrUsed] = (u32)kr_words0(R, links);
  }
}

// the new tiles (one lane per node), the records' buckets, the pass-0 records' frontier nodes, and what the receivers' brick / grid marks
// need from the records: the bricks whose node this commit created (their childless siblings get their lines: pool_grid.hip
// brick_siblings) and the keys of splits above the grid's block level (they re-label a whole cube)
__global__ __launch_bounds__(256) void keyrange_pack_tiles_kernel(u32 *__restrict__ delta, const u32 *__restrict__ pool,
                                                                  const unsigned long long *__restrict__ shadow, u32 epoch,
                                                                  const u64 *__restrict__ rec_key, const u32 *__restrict__ rec_front,
                                                                  const unsigned char *__restrict__ rec_pass, int brick_shift) {
  if (delta[kKrOverflow]) return;
  const u32 R = delta[kKrRecords], links = delta[kKrLinks], n0 = delta[kKrN0];
  unsigned char *bid = reinterpret_cast<unsigned char *>(delta + kr_bid0(R));
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < 8 * (size_t)R; i += (size_t)gridDim.x * 256u) {
    const u32 r = (u32)(i >> 3), q = (u32)(i & 7u);
    const u32 node = n0 + 8u * r + q;
    const unsigned long long sh = shadow[node];
    const u32 w0 = pool[2 * (size_t)node], w1 = (u32)(sh >> 32) == epoch ? (u32)sh : pool[2 * (size_t)node + 1];
    reinterpret_cast<uint2 *>(delta + kKrTiles0)[i] = make_uint2(w0, w1);
    if (q == 0u) {
      const u64 key = rec_key[r];
      const int d = (63 - __clzll((long long)key)) / 3, pass = rec_pass[r];
      bid[r] = (unsigned char)bucket_id(pass, d);
      if (r < links) delta[kr_links0(R) + r] = rec_front[r];
      if (d < kKrLevel) {  // a record several ranks may hold: listed by key for the union numbering
        const u32 pos = atomicAdd(&delta[kKrTop], 1u);
        if (pos < (u32)kKrTopCap) {
          u32 *e = delta + kKrTop0 + 4 * pos;
          e[0] = (u32)key; e[1] = (u32)(key >> 32); e[2] = r; e[3] = bucket_id(pass, d);
        }
      }
      if (d < kPoolGridBlockLevel) {
        const u32 pos = atomicAdd(&delta[kKrShallow], 1u);
        if (pos < (u32)kKrShallowCap) reinterpret_cast<u64 *>(delta + kKrHeader + kKrSibCap)[pos] = key;
      }
      if (brick_shift >= 0 && d == brick_node_level(brick_shift) && pass >= 1) {
        u32 x = 0, y = 0, z = 0;
        for (int k = 1; k <= d; k++) {
          const u32 oct = (u32)(key >> (3 * (d - k))) & 7u;
          x = (x << 1) | (oct & 1u); y = (y << 1) | ((oct >> 1) & 1u); z = (z << 1) | (oct >> 2);
        }
        const u32 org = brick_window_origin(brick_shift) >> 2;
        x -= org; y -= org; z -= org;
        if ((x | y | z) < (kBrickWindowCells >> 2)) {
          const u32 pos = atomicAdd(&delta[kKrSib], 1u);
          if (pos < (u32)kKrSibCap) delta[kKrHeader + pos] = brick_list_entry(x, y, z);
        }
      }
    }
  }
}

// {node, colour word} of the EXISTING nodes (below the pool's size) this commit changed: the leaf kernel's per-workgroup lists, then the
// straddler list (workgroups past the lists take 2048 entries each).  A workgroup counts, reserves with one atomic, writes.
__global__ __launch_bounds__(256) void keyrange_pack_words_kernel(u32 *__restrict__ delta, const unsigned long long *__restrict__ shadow,
                                                                  const u32 *__restrict__ apply_nodes, int fill_tiles, int list_cap,
                                                                  const u32 *__restrict__ strad, int strad_first, int strad_end) {
  if (delta[kKrOverflow]) return;
  __shared__ u32 wave_cnt[4], base_s;
  const u32 R = delta[kKrRecords], links = delta[kKrLinks], n0 = delta[kKrN0], cap = delta[kKrCapacity];
  const int t = (int)blockIdx.x, tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const bool lists = t < fill_tiles;
  const u32 *src; u32 cnt, stride;
  if (lists) { src = apply_nodes + (size_t)t * list_cap; cnt = apply_nodes[(size_t)fill_tiles * list_cap + t]; stride = 1u; }
  else {
    const long long first = strad_first + (long long)(t - fill_tiles) * 2048;
    src = strad + 2 * first; stride = 2u;
    const long long left = (long long)strad_end - first;
    cnt = left <= 0 ? 0u : (left < 2048 ? (u32)left : 2048u);
  }
  auto wanted = [&](u32 i) { if (i >= cnt) return false; const u32 node = src[(size_t)i * stride]; return node != kNoStraddler && node < n0; };
  u32 mine = 0;
  for (u32 i = (u32)tid; i < cnt; i += 256u) mine += wanted(i) ? 1u : 0u;
  u32 incl = mine;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) { const u32 v = __shfl_up(incl, o); if (lane >= o) incl += v; }
  if (lane == 63) wave_cnt[wave] = incl;
  __syncthreads();
  u32 before = 0, total = 0;
  for (int w = 0; w < 4; w++) { if (w < wave) before += wave_cnt[w]; total += wave_cnt[w]; }
  if (tid == 0) base_s = total ? atomicAdd(&delta[kKrWords], total) : 0u;
  __syncthreads();
  if (!total) return;
  const size_t w0 = kr_words0(R, links);
  if (w0 + 2 * ((size_t)base_s + total) > (size_t)cap) { if (tid == 0) delta[kKrOverflow] = 1u; return; }
  u32 pos = base_s + before + incl - mine;
  for (u32 i = (u32)tid; i < cnt; i += 256u)
    if (wanted(i)) {
      const u32 node = src[(size_t)i * stride];
      delta[w0 + 2 * (size_t)pos] = node;
      delta[w0 + 2 * (size_t)pos + 1] = (u32)shadow[node];
      pos++;
    }
  if (tid == 0) atomicMax(&delta[kKrUsed], (u32)(w0 + 2 * ((size_t)base_s + total)));
}

struct KrDeltas { const u32 *d[kKrMaxWorld]; };

// numbering: table[s][b] = what to add to rank s's local record rank in bucket b (depth >= 3) to get its place in the reference's order;
// topmap[s] = {count, then (local record, place) pairs} for rank s's records above the splitter level, ranked in the ranks' union; the
// union's tiles cleared; scal[0] = records of all ranks (shared ones once), [1] = status flags, [2] = first new tile, [3] = any valid key
constexpr int kKrTopMax = kKrMaxWorld * kKrTopCap;
__global__ __launch_bounds__(256) void keyrange_setup_kernel(KrDeltas D, int world, int *__restrict__ table, u32 *__restrict__ topmap,
                                                             u32 *__restrict__ scal, u32 *__restrict__ pool) {
  __shared__ unsigned tmp[4];
  __shared__ u64 top_key[kKrTopMax];
  __shared__ unsigned short top_bs[kKrTopMax];   // bucket | rank << 8
  __shared__ unsigned char top_first[kKrTopMax];
  __shared__ u32 top_base[kKrMaxWorld + 1], union_cnt[256];
  const int b = (int)threadIdx.x;
  u32 tot = 0, flags = 0, any = 0;
  union_cnt[b] = 0u;
  if (b == 0) {
    u32 run = 0;
    for (int s = 0; s < world; s++) { top_base[s] = run; const u32 c = D.d[s][kKrTop]; run += c < (u32)kKrTopCap ? c : (u32)kKrTopCap; }
    top_base[world] = run;
  }
  __syncthreads();
  const int M = (int)top_base[world];
  for (int s = 0; s < world; s++) {
    if (D.d[s][kKrOverflow] || D.d[s][kKrTop] > (u32)kKrTopCap) flags |= kKrOverflowed;
    if (D.d[s][kKrN0] != D.d[0][kKrN0] || D.d[s][kKrMagic] != 0x4B52414Eu) flags |= kKrMismatch;
    any |= D.d[s][kKrAnyValid];
    const int cnt = (int)(top_base[s + 1] - top_base[s]);
    for (int i = b; i < cnt; i += 256) {
      const u32 *e = D.d[s] + kKrTop0 + 4 * i;
      top_key[top_base[s] + i] = ((u64)e[1] << 32) | e[0];
      top_bs[top_base[s] + i] = (unsigned short)(e[3] | ((u32)s << 8));
    }
  }
  __syncthreads();
  // the union: an entry is its record's FIRST occurrence when no earlier entry holds the same (bucket, key)
  for (int e = b; e < M; e += 256) {
    bool first = true;
    for (int f = 0; f < e && first; f++) first = !(top_key[f] == top_key[e] && (top_bs[f] & 255u) == (top_bs[e] & 255u));
    top_first[e] = first ? 1 : 0;
    if (first) atomicAdd(&union_cnt[top_bs[e] & 255u], 1u);
  }
  __syncthreads();
  const int d = (b & 15) + 1;  // bucket_id(p, d) = 16 p + d - 1
  if (d < kKrLevel) tot = union_cnt[b];
  else for (int s = 0; s < world; s++) tot += D.d[s][256 + b];
  unsigned total;
  const u32 gbase = block256_exclusive_scan(tot, tmp, total);
  __shared__ u32 gbase_s[256];
  gbase_s[b] = gbase;
  u32 lower = 0;
  for (int s = 0; s < world; s++) {
    const u32 c = D.d[s][256 + b];
    unsigned ltot;
    const u32 lbase = block256_exclusive_scan(c, tmp, ltot);
    table[s * 256 + b] = (int)(gbase + lower) - (int)lbase;
    lower += c;
  }
  __syncthreads();
  const u32 n0 = D.d[0][kKrN0];
  for (int e = b; e < M; e += 256) {
    const u32 bk = top_bs[e] & 255u, s = top_bs[e] >> 8;
    u32 rank = 0;  // first occurrences of the bucket with a smaller key
    for (int f = 0; f < M; f++) rank += (top_first[f] && (top_bs[f] & 255u) == bk && top_key[f] < top_key[e]) ? 1u : 0u;
    const u32 place = gbase_s[bk] + rank;
    const u32 slot = (u32)e - top_base[s];
    topmap[s * (1 + 2 * kKrTopCap) + 1 + 2 * slot] = D.d[s][kKrTop0 + 4 * slot + 2];
    topmap[s * (1 + 2 * kKrTopCap) + 2 + 2 * slot] = place;
    if (top_first[e] && !flags) {  // the shared tile starts as eight empty children; the ranks then write what they filled
      uint4 *tile = reinterpret_cast<uint4 *>(pool + 2 * ((size_t)n0 + 8 * (size_t)place));
      const uint4 init = make_uint4(0u, kKrEmpty1, 0u, kKrEmpty1);
      tile[0] = init; tile[1] = init; tile[2] = init; tile[3] = init;
    }
  }
  if (b < world) topmap[b * (1 + 2 * kKrTopCap)] = top_base[b + 1] - top_base[b];
  if (flags) atomicOr(&scal[1], flags);
  if (b == 0) { scal[0] = total; scal[2] = n0; scal[3] = any; }
}

// every delta to its global place (blockIdx.y = the delta's rank): tiles with their links renumbered, the pass-0 links, the colour words
// of existing nodes, and the record-borne marks (sibling ring, cubes of shallow splits) into this replica's dirty state
__global__ __launch_bounds__(256) void keyrange_apply_kernel(KrDeltas D, const int *__restrict__ table, const u32 *__restrict__ topmap,
                                                             const u32 *__restrict__ scal, u32 *__restrict__ pool, u32 *__restrict__ dirty) {
  if (scal[1]) return;  // overflowed / mismatching deltas: nothing is applied (svo_fuse_keyrange_status reports it)
  const int s = (int)blockIdx.y;
  const u32 *delta = D.d[s];
  const int *T = table + s * 256;
  const u32 *tm = topmap + s * (1 + 2 * kKrTopCap);
  const u32 R = delta[kKrRecords], links = delta[kKrLinks], words = delta[kKrWords], n0 = delta[kKrN0];
  const unsigned char *bid = reinterpret_cast<const unsigned char *>(delta + kr_bid0(R));
  auto shared_record = [&](u32 r) { return (int)(bid[r] & 15u) + 1 < kKrLevel; };
  auto place = [&](u32 r) {
    if (shared_record(r)) {  // ranked in the ranks' union (a handful per frame, in the first frames of a map)
      const u32 cnt = tm[0];
      for (u32 i = 0; i < cnt; i++) if (tm[1 + 2 * i] == r) return tm[2 + 2 * i];
      return 0u;
    }
    return (u32)((int)r + T[bid[r]]);
  };
  const size_t stride = (size_t)gridDim.x * 256u, t0 = (size_t)blockIdx.x * 256u + threadIdx.x;
  for (size_t i = t0; i < 8 * (size_t)R; i += stride) {
    const u32 r = (u32)(i >> 3), q = (u32)(i & 7u);
    uint2 w = reinterpret_cast<const uint2 *>(delta + kKrTiles0)[i];
    if (shared_record(r) && w.x == 0u && w.y == kKrEmpty1) continue;  // a node of a shared tile this rank did not fill
    if (w.x & kFlag) w.x = kFlag | ((n0 + 8u * place(((w.x & kMask) - n0) >> 3)) & kMask);
    reinterpret_cast<uint2 *>(pool)[(size_t)n0 + 8 * (size_t)place(r) + q] = w;
  }
  for (size_t r = t0; r < links; r += stride) pool[2 * (size_t)delta[kr_links0(R) + r]] = kFlag | ((n0 + 8u * place((u32)r)) & kMask);
  const size_t w0 = kr_words0(R, links);
  for (size_t i = t0; i < words; i += stride) pool[2 * (size_t)delta[w0 + 2 * i] + 1] = delta[w0 + 2 * i + 1];
  if (dirty) {
    const u32 sib = delta[kKrSib] < (u32)kKrSibCap ? delta[kKrSib] : (u32)kKrSibCap;
    for (size_t i = t0; i < sib; i += stride) brick_sibling_list(dirty, delta[kKrHeader + i]);
    const u32 sh = delta[kKrShallow];
    if (sh > (u32)kKrShallowCap) {  // more shallow splits than the list holds: every block is stale
      for (size_t i = t0; i < (size_t)kPoolGridDirtyWords; i += stride) dirty[i] = 0xFFFFFFFFu;
    } else {
      for (size_t i = t0; i < sh; i += stride) {
        const u64 key = reinterpret_cast<const u64 *>(delta + kKrHeader + kKrSibCap)[i];
        pool_grid_mark(dirty, key, (63 - __clzll((long long)key)) / 3);
      }
    }
  }
}

// the marks of the ray march's level grid and occupancy bricks from ALL keys of the frame (as the leaf kernel makes them for the keys it
// commits: pool_grid.hpp), and the level-2 prefixes that occur (top[0..1]: a 64-bit mask) for the shared nodes' colour words
__global__ __launch_bounds__(256) void keyrange_mark_kernel(const u64 *__restrict__ skey, int n, int depth, u32 *__restrict__ dirty, int brick_shift,
                                                            unsigned long long *__restrict__ top) {
  __shared__ u32 brick_cnt, brick_base;
  __shared__ unsigned long long mask_s;
  const int tid = (int)threadIdx.x, j = (int)(blockIdx.x * 256u + threadIdx.x);
  if (tid == 0) { brick_cnt = 0u; mask_s = 0ull; }
  __syncthreads();
  u64 key = 1; int c = 0;
  const bool head = j < n && is_head(skey, j, key, c, depth);
  if (head && c < 2) atomicOr(&mask_s, 1ull << ((key >> (3 * (depth - 2))) & 63ull));
  if (dirty && head && c < kPoolGridBlockLevel) pool_grid_mark(dirty, key, depth);
  const bool bricks_on = dirty != nullptr && brick_shift >= 0 && depth >= brick_node_level(brick_shift);
  u32 entry = 0, off = 0;
  const bool mine = bricks_on && brick_mark_test(dirty, head && c < brick_node_level(brick_shift), key, depth, brick_shift, entry);
  const unsigned long long bm = __ballot(mine);
  if (bm) {
    const int leader = __ffsll((long long)bm) - 1;
    u32 woff = 0;
    if ((tid & 63) == leader) woff = atomicAdd(&brick_cnt, (u32)__popcll(bm));
    off = (u32)__shfl((int)woff, leader) + (u32)__popcll(bm & ((1ull << (tid & 63)) - 1ull));
  }
  __syncthreads();
  if (tid == 0) {
    if (brick_cnt) brick_base = brick_ring_reserve(dirty, brick_cnt);
    if (mask_s) atomicOr(top, mask_s);
  }
  __syncthreads();
  if (mine) brick_ring_store(dirty, brick_base + off, entry);
}

// keyrange_finish_kernel -- one workgroup, behind everything else: the colour words of the shared nodes, the root pass, the pool's size and
// its readback, the list of the marked grid blocks -- is defined in svo_build.hip, next to the straddler kernels whose tail it repeats.
// average_tile and pool_grid_compact are inlined into it, and the compiler specialises both on the arguments of the call sites it sees in
// a translation unit: compiled here, apart from those kernels, it comes out as other code (DESIGN.md lesson 4).

static int kr_scratch(svoslam_workspace *ws, int n) {  // slice arrays + window / table / scalars (zeroed once)
  SVO_TRY(ws->kr_keys.reserve((size_t)n * 8));
  SVO_TRY(ws->kr_idx.reserve((size_t)n * 4));
  if (ws->kr_small.bytes < 65536) {
    SVO_TRY(ws->kr_small.reserve(65536));
    SVO_HIP(memset_sync(ws->kr_small.ptr, 0, ws->kr_small.bytes));
  }
  return SVOSLAM_OK;
}
static inline int *kr_win(svoslam_workspace *ws) { return ws->kr_small.as<int>(); }                       // [0..3] window, [4..4+world] cuts
static inline u32 *kr_scal(svoslam_workspace *ws) { return ws->kr_small.as<u32>() + 64; }                 // setup scalars
static inline unsigned long long *kr_top(svoslam_workspace *ws) { return reinterpret_cast<unsigned long long *>(ws->kr_small.as<u32>() + 96); }
static inline int *kr_table(svoslam_workspace *ws) { return ws->kr_small.as<int>() + 128; }               // [world][256]
static inline u32 *kr_topmap(svoslam_workspace *ws) { return ws->kr_small.as<u32>() + 128 + kKrMaxWorld * 256; }  // [world][1 + 2 x kKrTopCap]

int svo_fuse_keyrange_commit(svoslam_workspace *ws, const unsigned long long *d_keys, const uint32_t *d_idx, const uint8_t *d_colors, int n,
                             int depth, svoslam_pool *pool, int rank, int world, uint32_t *d_delta, long long delta_bytes, hipStream_t stream) {
  if (!ws || !pool || !d_delta || n <= 0 || !d_keys || !d_idx || !d_colors) return SVOSLAM_ERR_INVALID_ARG;
  if (world < 1 || world > kKrMaxWorld || rank < 0 || rank >= world) return SVOSLAM_ERR_INVALID_ARG;
  if (depth < kKrLevel + 3 || depth > SVOSLAM_MAX_DEPTH) return SVOSLAM_ERR_DEPTH;
  if (delta_bytes < (long long)(kKrTiles0 + 64) * 4) return SVOSLAM_ERR_INVALID_ARG;
  SVO_TRY(kr_scratch(ws, n));
  int *win = kr_win(ws);
  keyrange_bounds_kernel<<<1, 64, 0, stream>>>(d_keys, n, depth, rank, world, win);
  keyrange_slice_kernel<<<cdiv(n, 256), 256, 0, stream>>>(d_keys, d_idx, n, win, ws->kr_keys.as<u64>(), ws->kr_idx.as<u32>());
  SVO_LAUNCH_CHECK();
  SVO_TRY(svo_fuse_adopt_sorted(ws, ws->kr_keys.as<u64>(), ws->kr_idx.as<u32>(), n, depth));
  SVO_TRY(svo_fuse_plan(ws, n, depth, pool, stream));
  SVO_TRY(commit_impl(ws, d_colors, n, depth, pool, true, stream, win + 2));
  // the delta
  unsigned long long *shadow = nullptr;
  u32 epoch = 0;
  SVO_TRY(pool_shadow_current(pool, &shadow, &epoch));
  int brick_shift = -1;
  (void)pool_accel_dirty_bitmap(pool, 0, depth, &brick_shift);  // (the shape this pool's bricks have, or will have, at this depth)
  if (depth < brick_node_level(brick_shift < 0 ? 0 : brick_shift)) brick_shift = -1;
  const int fill_tiles = ws->deferred_tiles;
  const long long rmax = max_records(n, depth);
  int tile_blocks = (int)cdiv(8 * rmax, 256);
  if (tile_blocks > 4096) tile_blocks = 4096;
  const int strad_first = fill_tiles, strad_end = depth * fill_tiles;
  const int strad_blocks = (int)cdiv((long long)strad_end - strad_first, 2048);
  keyrange_pack_header_kernel<<<1, 256, 0, stream>>>(d_delta, delta_bytes / 4, small_bucket_base(ws), small_counts(ws), small_n0(ws), win, depth);
  keyrange_pack_tiles_kernel<<<tile_blocks, 256, 0, stream>>>(d_delta, pool->d_data, shadow, epoch, ws->rec_key.as<u64>(), ws->rec_front.as<u32>(),
                                                              ws->rec_pass.as<unsigned char>(), brick_shift);
  keyrange_pack_words_kernel<<<fill_tiles + strad_blocks, 256, 0, stream>>>(d_delta, shadow, ws->apply_nodes.as<u32>(), fill_tiles, kFillThreads * depth,
                                                                            ws->strad.as<u32>(), strad_first, strad_end);
  SVO_LAUNCH_CHECK();
  pool_shadow_end(pool);
  ws->deferred_pool = nullptr;
  ws->keyrange_pool = pool;
  return SVOSLAM_OK;
}

int svo_fuse_keyrange_apply(svoslam_workspace *ws, const unsigned long long *d_keys, int n, int depth, svoslam_pool *pool,
                            const uint32_t *const *d_deltas, int world, hipStream_t stream) {
  if (!ws || !pool || !d_deltas || !d_keys || n <= 0 || world < 1 || world > kKrMaxWorld) return SVOSLAM_ERR_INVALID_ARG;
  if (ws->keyrange_pool != pool) return SVOSLAM_ERR_INVALID_ARG;  // svo_fuse_keyrange_commit of this frame has not run on this workspace
  ws->keyrange_pool = nullptr;
  KrDeltas D;
  for (int s = 0; s < kKrMaxWorld; s++) D.d[s] = s < world ? d_deltas[s] : nullptr;
  for (int s = 0; s < world; s++) if (!D.d[s]) return SVOSLAM_ERR_INVALID_ARG;
  PoolTracker *trk = tracker_of(pool);
  int brick_shift = -1;
  u32 *dirty = pool_accel_dirty_bitmap(pool, 0, depth, &brick_shift);  // direct-commit state; nullptr: not a registered pool
  const long long rmax = max_records(n, depth);
  int blocks = (int)cdiv(8 * rmax / (world > 1 ? world : 1) + 1, 256);
  if (blocks > 2048) blocks = 2048;
  if (blocks < 64) blocks = 64;
  keyrange_setup_kernel<<<1, 256, 0, stream>>>(D, world, kr_table(ws), kr_topmap(ws), kr_scal(ws), pool->d_data);
  keyrange_apply_kernel<<<dim3((unsigned)blocks, (unsigned)world), 256, 0, stream>>>(D, kr_table(ws), kr_topmap(ws), kr_scal(ws), pool->d_data, dirty);
  keyrange_mark_kernel<<<cdiv(n, 256), 256, 0, stream>>>(d_keys, n, depth, dirty, brick_shift, kr_top(ws));
  SVO_TRY(tracker_make_room(pool));
  keyrange_finish_kernel<<<1, 256, 0, stream>>>(pool->d_data, kr_scal(ws), kr_top(ws), pool->d_size, trk ? trk->h_size : nullptr,
                                                trk ? trk->d_slot : nullptr, dirty);
  SVO_LAUNCH_CHECK();
  pool->pending += 1;
  return tracker_push(pool, ws->keyrange_bound, stream);
}

// a svo_fuse_keyrange_commit whose delta is wanted but whose apply will not follow on this pool (the deltas of OTHER ranks, produced on one
// device for an emulated rank: bench.py --exchange keyrange --emulate-rank): the plan's reservation is released, the pool is as it was
int svo_fuse_keyrange_discard(svoslam_workspace *ws, svoslam_pool *pool) {
  if (!ws || !pool || ws->keyrange_pool != pool) return SVOSLAM_ERR_INVALID_ARG;
  ws->keyrange_pool = nullptr;
  pool->pending_bound -= ws->keyrange_bound;
  if (pool->pending_bound < 0) pool->pending_bound = 0;
  return SVOSLAM_OK;
}

// flags of the svo_fuse_keyrange_apply calls on this workspace since the last call of this function (blocking; the flags are sticky on
// the device and cleared here): 0 = every frame applied; kKrOverflowed / kKrMismatch = a frame was NOT applied (the replica
// is then behind the others)
int svo_fuse_keyrange_status(svoslam_workspace *ws, int *flags, hipStream_t stream) {
  if (!ws || !flags || ws->kr_small.bytes == 0) return SVOSLAM_ERR_INVALID_ARG;
  u32 f = 0;
  SVO_HIP(hipMemcpyAsync(&f, kr_scal(ws) + 1, 4, hipMemcpyDeviceToHost, stream));
  SVO_HIP(hipStreamSynchronize(stream));
  *flags = (int)f;
  if (f) SVO_HIP(memset_sync(kr_scal(ws) + 1, 0, 4));
  return SVOSLAM_OK;
}

}  // namespace svoslam
