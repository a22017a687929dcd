// map_reach.hpp -- the reach field of a map region: shortest free-path steps from seed cells (map_reach.hip; own specification,
// DESIGN.md section 16)
#pragma once
#include <functional>

#include "common.hpp"
#include "map_region.hpp"
#include "map_relax.hpp"
#include "stage_timing.hpp"

namespace svoslam {
int pool_reach_field(svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3], const int32_t dims[3],
                     int32_t clearance_cells, const int32_t *d_seeds, int32_t n_seeds, int32_t *d_steps, svoslam_reach_stats *stats,
                     hipStream_t stream);

// what a reach relaxation works on: the region, its tiles, and the workspace's two reach slots
struct ReachFrame {
  RegionPlan own;            // the region itself (R = 0); own.nothing: a side is 0 cells and nothing was launched
  TileGrid g;
  long long tiles;
  unsigned long long *bits;  // T's row words
  RelaxControl *ctl;         // all zero when the seeding starts
  int *flags;                // round 0's and round 1's, all clear when the seeding starts; then `spare` ints per tile of the caller's
};

// pool_reach_field with the seeding left to the caller (the owner field's, map_owner.hip, is another): the checks and limits, the
// distance field into d_steps under the bracket it opens into `bracket`, the slots, the pack, seed(frame) -- which writes 0 at its
// counted seeds, counts them in ctl->seeds_used and raises round 0's flags -- then the rounds of reach_relax_kernel and the finish.
// The caller has checked ws and the seeds' arguments.  `spare`: ints per tile that the flag slot holds beyond the two rounds' flags.
int reach_relax(const char *fn, svoslam_workspace *ws, const svoslam_pool *pool, int depth, const int32_t origin[3],
                const int32_t dims[3], int32_t clearance_cells, int32_t *d_steps, int spare,
                const std::function<int(const ReachFrame &)> &seed, AdoptedBracket &bracket, ReachFrame *frame, long long *rounds,
                RelaxControl *seen, hipStream_t stream);
}  // namespace svoslam
