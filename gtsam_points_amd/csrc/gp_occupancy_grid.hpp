// gp_occupancy_grid.hpp -- the host side of the occupancy set (gp_occupancy.hip): the grid behind the gp_occupancy_grid_* entry points, and the three functions its
// one internal client calls -- RANSAC (gp_registration.hip) builds the target's grid and scores against it on its own stream, without a wait.  The device side
// (cell, key, lookup) is gp_occupancy.hpp.
#pragma once

#include "gp_host.hpp"
#include "gp_occupancy.hpp"

struct gp_occupancy_grid {
  double resolution = 1.0;
  hipStream_t stream = nullptr;
  gp::DeviceArray keys;      // unsigned long long[slots]
  gp::DeviceArray words;     // uint32_t[slots][16]
  gp::DeviceArray counters;  // int[2]: occupied blocks, occupied cells
  uint32_t slots = 0;
  int num_blocks = 0;
  int num_cells = 0;
  ~gp_occupancy_grid() {  // the arrays are pooled blocks that any stream may take next: the work that reads them finishes first
    if (keys.ptr) (void)hipStreamSynchronize(stream);
  }
  gp::OccupancyView view() const {
    gp::OccupancyView v;
    v.keys = keys.as<unsigned long long>();
    v.words = words.as<uint32_t>();
    v.mask = slots - 1;
    v.pad_ = 0;
    v.inv_resolution = 1.0 / resolution;
    return v;
  }
};

namespace gp {

// an empty grid on `stream` with room for reserve_points points
int grid_init(gp_occupancy_grid* g, double resolution, hipStream_t stream, int reserve_points = 0);
// wait: read the counts back (one synchronisation); without it the insert is only queued and num_blocks / num_cells stay as they were
int grid_insert(gp_occupancy_grid* g, const float* points, int n, const double* pose, bool wait = true);
// the scoring launch (occupancy_overlap_batch_kernel): counts[h] += the points of the cloud whose cell at poses_dev[h] is in the set, for h = list[slot] (list NULL:
// h = slot), slot < *num_list (NULL: num_slots); stop: a device flag read first, or NULL.  Asynchronous on `stream`.
int launch_overlap_batch(const gp_occupancy_grid* grid, const float* points, int n, const double* poses_dev, const int* list, const int* num_list, int num_slots, const int* stop,
                         int* counts, hipStream_t stream);

}  // namespace gp
