// map_region.hpp -- what the region fields share on the host (map_region.hip): the plan of a region of cells
// inflated by a radius and clipped to the root, its raster into bit rows, the exact truncated distance transform of those rows, the
// packing of a field's -1 into bit rows of the region itself, and the rollback of the workspace slots a failed call grew
#pragma once
#include <initializer_list>

#include "workspace.hpp"

namespace svoslam {

struct RegionPlan {
  long long lo[3], len[3];  // the inflated region: first cell and cells per axis
  int off[3];               // the region's first cell inside the inflated one
  long long nx, ny, nz, n_out;
  long long wpr, words;     // 64-bit words per row of the inflated region, and in all its rows
  long long n_g1, n_g2;     // values after the transform's x pass [len z][len y][nx] and after its y pass [len z][ny][nx]
  bool nothing;             // a side of the region is 0 cells: the call is done
};

// SVOSLAM_ERR_INVALID_ARG unless 1 <= depth <= SVOSLAM_MAX_DEPTH, 0 <= R <= SVOSLAM_MAX_RADIUS_CELLS and the region lies in the root
int plan_region(int depth, const int32_t origin[3], const int32_t dims[3], int R, RegionPlan *plan);
// the same with an inflation per axis and side: `below[a]` cells towards smaller and `above[a]` towards larger coordinates, each in
// 0..SVOSLAM_MAX_RADIUS_CELLS.  n_g1 and n_g2 are those of region_transform_planar along `pass_axis` (1 or 2): the axis other than
// x and pass_axis is not transformed and keeps its inflated length -- g1 [len z][len y][nx], g2 the same with pass_axis cut to the
// region
int plan_region_axes(int depth, const int32_t origin[3], const int32_t dims[3], const int below[3], const int above[3], int pass_axis,
                     RegionPlan *plan);
// what follows a caller's own argument checks: the pool, the 2^31 - 1 limits (worded for the public function `fn`; `transform`:
// those of region_transform's intermediates too), then the drain of pending asynchronous fusions
int admit_region(const char *fn, const svoslam_pool *pool, const RegionPlan &p, int R, bool transform, hipStream_t stream);

// bits[p.words]: bit x of a row = the cell is occupied, or, with `complement`, is a cell of the row that is not
int region_raster(const svoslam_pool *pool, int depth, const RegionPlan &p, bool complement, unsigned long long *bits,
                  hipStream_t stream);

struct LaunchEvents {  // the profiling form's events: mark() in front of each launch and once behind the last
  hipEvent_t ev[5] = {};
  int n = 0;
  int mark(hipStream_t stream);
  ~LaunchEvents();
};

// x, y and z pass over the raster: g1[p.n_g1], g2[p.n_g2], out[p.n_out] (-1: nothing within R).  With wx, each pass also writes
// where its minimum lies, the smallest index among the equally near: wx[p.n_g1], ay[p.n_g2], az[p.n_out]; else all three are NULL
int region_transform(const RegionPlan &p, int R, const unsigned long long *bits, int32_t *g1, int32_t *g2, int32_t *out, uint16_t *wx,
                     uint16_t *ay, uint16_t *az, hipStream_t stream, LaunchEvents *timed = nullptr);

// the planar transform of a plan_region_axes plan: edt_x_kernel, then one column pass along pass_axis; the third axis is left alone,
// so out[p.n_g2] holds, per layer of that axis, the squared distance within the layer (-1: nothing within R)
int region_transform_planar(const RegionPlan &p, int R, int pass_axis, const unsigned long long *bits, int32_t *g1, int32_t *out,
                            hipStream_t stream);
// the 2^31 - 1 limits of region_transform_planar's intermediates and launches
bool planar_within_limits(const RegionPlan &p, int pass_axis);

// `own`: the plan of the region with R = 0.  bits[own.words]: bit x of a row = (values == -1) != invert; with `none`, every value
// is then overwritten with *none
int region_pack(const RegionPlan &own, int32_t *values, bool invert, const int *none, unsigned long long *bits, hipStream_t stream);

// what a call grew of the listed slots (at most 6; a NULL entry is skipped) does not stay behind a failure
struct SlotRollback {
  DeviceBuffer *slots[6];
  size_t had[6];
  int n = 0;
  SlotRollback(std::initializer_list<DeviceBuffer *> list) {
    for (DeviceBuffer *slot : list)
      if (slot && n < 6) {
        slots[n] = slot;
        had[n++] = slot->bytes;
      }
  }
  // pool_distance_field's slots first, then the caller's own two or three
  SlotRollback(svoslam_workspace *ws, DeviceBuffer *own_a, DeviceBuffer *own_b, DeviceBuffer *own_c = nullptr)
      : SlotRollback({&ws->field_bits, &ws->field_a, &ws->field_b, own_a, own_b, own_c}) {}
  int undo(int rc, hipStream_t stream) {  // the field's launches have finished before their slots go
    (void)hipStreamSynchronize(stream);
    for (int k = 0; k < n; k++)
      if (slots[k]->bytes != had[k]) slots[k]->release();
    return rc;
  }
};

}  // namespace svoslam
