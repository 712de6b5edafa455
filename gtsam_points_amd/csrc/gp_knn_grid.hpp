// gp_knn_grid.hpp -- the structures an exact k-NN search runs on (gp_knn.hip builds them, gp_knn_search.hpp walks them, gp_covariance.hip builds one per call):
// the hashed multi-level grid (GridView / MultiGridView: keys, cell starts and the cell-sorted points of up to kMaxLevels levels), the binned grid
// (BinGridView: the occupancy blocks of gp_binning.hpp + the cell-sorted points + the superblock masks), SearchView (what a kernel is handed: one or
// the other), and the host structs that own their device arrays (gp_grid_level, gp_point_grid; gp_point_grid stays private to the library).
//
// Replaces (reference, CPU only): the tree that KdTreeBuilder builds (ann/small_kdtree.hpp:124-186) -- a uniform grid instead of a kd-tree.
#pragma once

#include <memory>
#include <vector>

#include "gp_binning.hpp"
#include "gp_host.hpp"
#include "gp_key_table.hpp"

namespace gp {

__host__ __device__ __forceinline__ unsigned long long pack_cell(int x, int y, int z) {
  return ((unsigned long long)(unsigned)(x + (1 << 20)) << 42) | ((unsigned long long)(unsigned)(y + (1 << 20)) << 21) | (unsigned long long)(unsigned)(z + (1 << 20));
}

// cell coordinate of the hashed grid: 21-bit fields.  Coordinates beyond +-2^20 cells are clamped to the border cells and a
// non-finite coordinate goes to cell 0: such points sit in a cell that is never FARTHER from a query than their true cell, so the
// shell search still meets them in time (distances always come from the real coordinates; NaN / inf distances are never selected)
__host__ __device__ __forceinline__ int hashed_cell(double u) {
  if (!cell_in_range(u)) return 0;  // (the cell rule's range test: gp_cells.hpp)
  const int c = fast_floor(u);
  const int lim = (1 << 20) - 3;
  return c < -lim ? -lim : (c > lim ? lim : c);
}

struct GridView {
  const unsigned long long* keys;  // [slots] packed cell coordinate or kEmptyKey: a table of gp_key_table.hpp, home slot hash_key(key) & mask
  const int* start;                // [slots + 1] first sorted point of the cell stored at this slot
  const float4* sorted;            // [n] (x, y, z, original index as int bits), cell-sorted
  uint32_t mask;
  int n;
  double inv_h, h;
  int lo[3], hi[3];  // bounding box of the occupied cells: bounds the cube radius of any query
};

__device__ __forceinline__ int grid_find(const GridView& g, unsigned long long key) { return key_find(g.keys, g.mask, hash_key(key) & g.mask, key); }

// LiDAR density varies by three orders of magnitude between the near and the far field, so one cell size cannot be right
// everywhere: the structure keeps up to kMaxLevels grids (cell size x4 per level) and every query runs the same exact
// search on the finest level whose 3x3x3 neighbourhood already holds enough points.  Exactness does not depend on the choice.
constexpr int kMaxLevels = 3;
struct MultiGridView {
  GridView lv[kMaxLevels];
  int num_levels;
};

// the binned structure (gp_binning.hpp): occupancy-block grid over the cells + cell-sorted points (searched by knn_query_bins / knn_query_coarse, gp_knn_search.hpp)
struct BinGridView {
  const GridBlock* blocks;
  const int* cell_start;  // [num_cells + 1]
  const float4* sorted;   // [n] (x, y, z, original index as int bits), cell-major, ascending index inside a cell
  GridGeom geom;
  double inv_h, h;
  int n;  // binned (finite) points
  const unsigned long long* super;  // [sdim[2]][sdim[1]][sdim[0]] occupancy masks of 4 x 4 x 4 blocks, relative block coordinate >> 2
  int sdim[3];
  unsigned long long* counters;  // measurement build only (gp_debug_knn_counters): {queries, f32 distances, f64 distances, block entries, cells}
};

// what a search runs on: the binned structure, or -- for clouds whose bounding box is too large for it -- the hashed multi-level grid
// LiDAR density spans three orders of magnitude between the near and the far field: a query first tries the shells 0 and 1 of the
// cells (<= 8 block entries); when that does not settle it (sparse neighbourhood) it starts over on the blocks taken as cells four
// times the size, and then on the superblocks (knn_query_coarse), which it walks until the bound is met.  (More binned levels, cell size x4 each, can be stacked in
// between -- gp_debug_set_knn_structure -- but building them costs more than they save.)  Every stage is an exact search, so the
// staging affects speed only.
struct SearchView {
  int binned;      // number of binned levels (0: hashed fallback)
  int fine_shells; // shells beyond the first one that a query walks on the finest cells before it starts over on a coarser level (4 in rounds 2-3)
  int block_stage; // shells of BLOCKS (cells four times the size) a query walks between the fine shells and the superblocks; 0 = round 3's staging (none)
  BinGridView bins[kMaxLevels];
  MultiGridView hashed;
};

}  // namespace gp

struct gp_grid_level {
  gp::DeviceArray arena;  // one allocation: keys | start | sorted (device allocations cost far more than the build kernels)
  void *keys_p = nullptr, *start_p = nullptr, *sorted_p = nullptr;
  uint32_t mask = 0;
  int n = 0;
  double h = 0.0;
  int lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  gp::GridView view() const {
    gp::GridView g;
    g.keys = static_cast<const unsigned long long*>(keys_p);
    g.start = static_cast<const int*>(start_p);
    g.sorted = static_cast<const float4*>(sorted_p);
    g.mask = mask;
    g.n = n;
    g.h = h;
    g.inv_h = 1.0 / h;
    for (int a = 0; a < 3; a++) {
      g.lo[a] = lo[a];
      g.hi[a] = hi[a];
    }
    return g;
  }
};


struct gp_point_grid {
  // default: the binned structure (gp_binning.hpp) + the cell-sorted copy of the points, in up to kMaxLevels levels (cell x4 each)
  struct BinLevel {
    gp::PointBins bins;
    gp::DeviceArray sorted;  // float4[num_binned]
    gp::DeviceArray super;   // unsigned long long[sdim product]
    int sdim[3] = {0, 0, 0};
    double h = 0.0;
  };
  std::vector<std::unique_ptr<BinLevel>> bin_levels;
  bool binned = false;
  int num_binned = 0;
  // fallback for clouds whose bounding box is too large for the block grid: hashed multi-level grid
  std::vector<std::unique_ptr<gp_grid_level>> levels;
  hipStream_t stream = nullptr;
  int structure = 0;                       // GP_TUNE_KNN_STRUCTURE value the grid was created with (per structure, nothing process-global)
  unsigned long long* counters = nullptr;  // caller's device buffer of 8 work counters, or null (gp_point_grid_create_ex; measurement only)
  gp::SearchView view() const {
    gp::SearchView v{};
    v.binned = binned ? (int)bin_levels.size() : 0;
    // round 4 measured both knobs on the 1 M-point cloud (scripts/r04_c5.py, profiles/r04_c5_staging.jsonl): fine shells 0 .. 4 with and without two or three shells
    // of blocks in front of the superblocks -- 1.02-1.05 ms per call whatever the staging: 1434 of 10^6 queries get past the fine shells at all
    // (profiles/r04_c5_wavelog.txt).  The defaults stay round 3's.
    v.block_stage = 0;
    v.fine_shells = 4;
    if (structure >= 16) {  // experiment encoding (scripts/r04_c5.py): 16 | fine shells << 4 | block shells << 8
      v.fine_shells = (structure >> 4) & 7;
      v.block_stage = (structure >> 8) & 7;
    }
    if (binned) {
      for (size_t l = 0; l < bin_levels.size(); l++) {
        const BinLevel& b = *bin_levels[l];
        v.bins[l].blocks = b.bins.blocks.as<gp::GridBlock>();
        v.bins[l].cell_start = b.bins.cell_start.as<int>();
        v.bins[l].sorted = b.sorted.as<float4>();
        v.bins[l].geom = b.bins.geom;
        v.bins[l].inv_h = 1.0 / b.h;
        v.bins[l].h = b.h;
        v.bins[l].n = b.bins.num_binned;
        v.bins[l].super = b.super.as<unsigned long long>();
        for (int a = 0; a < 3; a++) v.bins[l].sdim[a] = b.sdim[a];
        v.bins[l].counters = counters;
      }
    } else {
      v.hashed.num_levels = (int)levels.size();
      for (int l = 0; l < v.hashed.num_levels; l++) v.hashed.lv[l] = levels[l]->view();
    }
    return v;
  }
  // for an owner that built and searched the structure on `s` alone: every device array goes back to the pool in that stream's order (the destructor returns them in
  // the order they were allocated with, which is safe only behind a synchronisation of everything that searched: gp_point_grid_destroy)
  void release_on(hipStream_t s) {
    for (auto& lv : bin_levels)
      for (gp::DeviceArray* a : {&lv->bins.blocks, &lv->bins.cell_start, &lv->bins.order, &lv->bins.cell_of, &lv->bins.cell_block, &lv->bins.occ_blocks, &lv->sorted, &lv->super})
        a->release_on(s);
    for (auto& lv : levels) lv->arena.release_on(s);
  }
};

namespace gp {
// the structure build behind gp_point_grid_create[_ex] and gp_estimate_covariances (gp_knn.hip)
// keep_cell_of: the cell ordinals of the sorted positions stay with the first level (gp_estimate_covariances orders its queries by them);
// synchronise = false: the caller searches on `stream` itself, the last kernels of the build need not be waited for
// caller_zero: a fill the caller wants done on the stream before it searches; it rides in one of the build's kernels when the binned build runs (*caller_zero_applied)
int point_grid_create_impl(const float* points_dev, int n, double cell_size, int structure, unsigned long long* counters_dev, gp_stream_t stream, bool keep_cell_of,
                           bool synchronise, gp_point_grid_t** out, const FillJob caller_zero = FillJob{}, bool* caller_zero_applied = nullptr);
}  // namespace gp
