// gp_voxelmap.hpp -- what the host units of the voxel map share: gp_voxelmap.hip (handle, the two builds, the block grid and bucket placement, the queries),
// gp_voxelmap_store.hip (download, assign, save / load, clone, offload / reload) and gp_voxelmap_incremental.hip (the incremental insert with LRU eviction).  The map itself is gp_voxelmap in gp_host.hpp, with
// the one table of its arrays.
#pragma once

#include "gp_binning.hpp"
#include "gp_host.hpp"

namespace gp {

constexpr int64_t kMaxBuckets = int64_t(1) << 30;  // entries of a bucket table: every doubling sequence ends here

// bounding box in block units before the first voxel: bbox[0..2] = min, bbox[3..5] = max
inline void empty_bbox(int bbox[6]) { CellBox().store(bbox); }  // (the neutral box: gp_cells.hpp)

// the six entries xx xy xz yy yz zz of a symmetric 3x3 <-> its nine entries
template <typename T>
inline void sym6_to_full(const T* r, T* c) {
  c[0] = r[0];
  c[1] = c[3] = r[1];
  c[2] = c[6] = r[2];
  c[4] = r[3];
  c[5] = c[7] = r[4];
  c[8] = r[5];
}
template <typename T>
inline void full_to_sym6(const T* c, T* r) {
  r[0] = c[0];
  r[1] = c[3];
  r[2] = c[6];
  r[3] = c[4];
  r[4] = c[7];
  r[5] = c[8];
}

// ---- gp_voxelmap.hip (between the two units only: kept out of the library's dynamic symbols) ----
#pragma GCC visibility push(hidden)
// geometry of the block grid from the block-unit bounding box; false when the box exceeds the budget (kMaxGridBlocks)
bool grid_geometry(const int bbox[6], GridGeom* g, long long* num_blocks);
// records, num_points, voxel_means, voxel_covs and voxel_intensities for info.num_voxels voxels, from the pool on the map's stream
int alloc_voxel_arrays(gp_voxelmap* m);
// ---- the pieces of a map build that the incremental insert shares; their kernels live in gp_voxelmap.hip (VoxelSet: gp_voxelmap_kernels.hpp) ----
struct VoxelSet;
// box[] (in: the box so far, out: joined with the block-unit box of the set's living voxels), through the six device ints bbox_dev.  Synchronises the stream
int voxels_bbox(const VoxelSet& set, int* bbox_dev, int box[6], hipStream_t s);
// the block grid of the sets' living voxels in blocks[nb]: zero -> mark -> count -> exclusive scan of the bases, which leaves the voxel count behind the block sums of
// scan_scratch (scan_scratch_ints(nb) ints, gp_scan.hpp).  Asynchronous on `s`; the caller allocates
int build_block_grid(const GridGeom& g, long long nb, GridBlock* blocks, int* scan_scratch, const VoxelSet* sets, int num_sets, hipStream_t s);
// the first size of the doubling sequence init, 2 init, ... that holds V voxels at the load factor
int64_t entry_bucket_count(int64_t init, int load_percent, int V);
// the bucket table of the V voxels at `coords`, doubled from *num_buckets until every voxel is placed (then *num_buckets is its size and the work on `s` is complete).
// The caller allocates the first table; first_table_prefilled: a kernel already on `s` fills it with "empty".  `api` names the caller in the 2^30-entries refusal
int place_voxels(const char* api, const int* coords, const int* num_points, int V, DeviceArray& buckets, int64_t* num_buckets, int max_scan, bool first_table_prefilled,
                 hipStream_t s);
// (re)build the line table of the hashed VGICP kernel family from the voxel list (line_claim_kernel: the one launch the storage unit asks for).  Asynchronous on `s`
int build_private_table(gp_voxelmap* m, hipStream_t s);
#pragma GCC visibility pop

}  // namespace gp
