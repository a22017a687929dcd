/* svoslam_corridor.h -- safe corridors along planned paths: chains of overlapping axis-aligned boxes of free cells over a distance
 * field.  An extension of svoslam.h with a header of its own; the functions live in the same library (libsvoslam_hip.so).
 *
 * Safe corridors (no reference counterpart; specification here and in DESIGN.md section 27): the last step of the planning chain
 * plan (svoslam_pool_cost_field, svoslam_field_trace_paths), straighten (svoslam_field_shorten_paths), corridor.  A box of free
 * cells is a convex set of six linear constraints, so a spline or MPC solver can take a chain of them as it stands.  Exact, in
 * integers.  No pool, no workspace; asynchronous on `stream`, nothing is read back; one SVOSLAM_STAGE_QUERY bracket around the one
 * launch of each call.
 *
 * Common definitions
 *   d_dist2, origin_cell, dims, g(c) and the limits of the region are exactly those of svoslam_field_shorten_paths' "Common
 *     definitions" (svoslam.h): at most 2^16 cells per axis and at most 2^31 - 1 cells in all; g is 0 for a cell outside the region,
 *     and no cell outside the region is read.
 *   r = clearance_cells, 0..SVOSLAM_MAX_RADIUS_CELLS.  A cell c is FREE iff g(c) > r^2; a free cell therefore lies in the region.  THE
 *     CALLER MUST SUPPLY A FIELD WHOSE RADIUS IS >= r, as for svoslam_field_shorten_paths; the call cannot check it.
 *   E = max_extent, 0..SVOSLAM_MAX_CORRIDOR_EXTENT: the most layers a box may grow in each of its six directions.
 *   A box is lo (x, y, z), hi (x, y, z) in absolute cells, both inclusive: 6 int32.
 *   grow(box) runs rounds.  In each round the six directions are tried in the order -x, +x, -y, +y, -z, +z.  A direction that has
 *     grown fewer than E layers grows by one layer iff every cell of the new layer is free; the new layer is the slab one cell thick
 *     beside that face of the box, spanning the box's CURRENT extent on the other two axes.  The box is updated at once: the later
 *     directions of the same round see it.  Growth stops after a round in which nothing grew.  By induction every cell of the
 *     result is free when every cell of the box was.  The result depends on the order of the directions; it is a box that no single
 *     layer can extend, not the largest free box.
 *
 * svoslam_field_grow_boxes
 *   d_seeds: n rows of 6 int32 in device memory, lo xyz then hi xyz, anywhere in int32.  A seed is VALID iff lo <= hi on every axis,
 *     it lies inside the region, and all its cells are free.
 *   Outputs: for a valid seed d_boxes[i] = grow(seed) and d_layers[i] = the layers added in total, 0..6E.  For any other seed
 *     d_boxes[i] = the seed as given and d_layers[i] = -1.  One wavefront per seed.
 *
 * svoslam_field_path_corridors
 *   d_paths, d_lengths, n_paths, max_cells: exactly as svoslam_field_shorten_paths reads them: path i has L = min(|d_lengths[i]|,
 *     max_cells) stored cells p_0 .. p_(L-1); any list of cells is accepted.
 *   Box of an anchor index a: if p_a is not free the box is EMPTY, stored as lo = p_a and hi = p_a - 1 on every axis (in int32
 *     arithmetic).  Otherwise the seed is {p_a}, and p_(a+1) joins it if a + 1 < L, p_(a+1) is a face neighbour of p_a and p_(a+1) is
 *     free; the box is grow(the bounding box of the seed).  The pair makes the box hold the next cell whatever the order of the
 *     directions does to a box grown from p_a alone.
 *   e(a) = the largest j >= a such that p_a .. p_j all lie in the box; a for an empty box.
 *   Anchors: a_0 = 0.  After an anchor a: stop if e(a) == L - 1; else the next anchor is e(a) if e(a) > a, and a + 1 otherwise.  The
 *     anchor rises strictly.
 *   Outputs: d_counts[i] = the number of anchors, EVEN WHEN IT EXCEEDS max_boxes; 0 for L = 0.  d_boxes [n_paths][max_boxes][6] and
 *     d_anchors [n_paths][max_boxes] receive the first min(count, max_boxes) boxes and anchor indices, the entries behind them are
 *     not written (both may be NULL if max_boxes == 0).  d_gaps[i] (may be NULL) = the number of anchors a with an empty box or with
 *     e(a) == a < L - 1: the places where the chain is broken.
 *   On a path of face-neighbour free cells -- what svoslam_field_trace_paths writes over a cost field of the same clearance -- gaps
 *     is 0, consecutive boxes share the cell p_(a_(k+1)), every path cell lies in a box, and every cell of every box is free.
 *   One wavefront per path.
 *
 * Errors of both calls, all decided before anything is written: SVOSLAM_ERR_INVALID_ARG: NULL origin_cell or dims; a negative entry
 *     of dims, n, n_paths, max_cells or max_boxes; clearance_cells outside 0..SVOSLAM_MAX_RADIUS_CELLS; max_extent outside
 *     0..SVOSLAM_MAX_CORRIDOR_EXTENT; with n > 0 a NULL d_seeds, d_boxes or d_layers; with n_paths > 0 a NULL d_lengths or d_counts, a
 *     NULL d_paths with max_cells > 0, a NULL d_boxes or d_anchors with max_boxes > 0; with work to do a NULL d_dist2 over a
 *     non-empty region.  SVOSLAM_ERR_POOL_LIMIT: the limits above, n_paths * max_cells * 3 > 2^31 - 1, or n_paths * max_boxes * 6 >
 *     2^31 - 1.  n == 0 / n_paths == 0 launches nothing.  A zero entry of dims is valid: no cell is free, so every seed is invalid and
 *     every box of a path is empty. */
#ifndef SVOSLAM_CORRIDOR_H_
#define SVOSLAM_CORRIDOR_H_

#include "svoslam.h"

#ifdef __cplusplus
extern "C" {
#endif

#define SVOSLAM_MAX_CORRIDOR_EXTENT 65536
int svoslam_field_grow_boxes(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells,
                             int32_t max_extent, const int32_t *d_seeds /* [n][6]: lo xyz, hi xyz */, int32_t n,
                             int32_t *d_boxes /* [n][6] */, int32_t *d_layers /* [n] */, void *stream);
int svoslam_field_path_corridors(const int32_t *d_dist2, const int32_t origin_cell[3], const int32_t dims[3], int32_t clearance_cells,
                                 int32_t max_extent, const int32_t *d_paths /* [n_paths][max_cells][3] */,
                                 const int32_t *d_lengths /* [n_paths] */, int32_t n_paths, int32_t max_cells, int32_t max_boxes,
                                 int32_t *d_boxes /* [n_paths][max_boxes][6], may be NULL if max_boxes == 0 */,
                                 int32_t *d_anchors /* [n_paths][max_boxes], may be NULL if max_boxes == 0 */,
                                 int32_t *d_counts /* [n_paths] */, int32_t *d_gaps /* [n_paths], may be NULL */, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* SVOSLAM_CORRIDOR_H_ */
