// gp_voxelmap.hpp -- what the host units of the voxel map share: gp_voxelmap.hip (handle, the two builds, the queries), gp_voxelmap_store.hip (download, assign,
// save / load, clone, offload / reload) and gp_voxelmap_incremental.hip (the incremental insert with LRU eviction).  The map itself is gp_voxelmap in gp_host.hpp, with
// the one table of its arrays.
#pragma once

#include "gp_binning.hpp"
#include "gp_host.hpp"

namespace gp {

constexpr int64_t kMaxBuckets = int64_t(1) << 30;  // entries of a bucket table: every doubling sequence ends here

// bounding box in block units before the first voxel: bbox[0..2] = min, bbox[3..5] = max
inline void empty_bbox(int bbox[6]) {
  for (int a = 0; a < 3; a++) {
    bbox[a] = 0x7fffffff;
    bbox[3 + a] = (int)0x80000000;
  }
}

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
// (re)build the line table of the hashed VGICP kernel family from the voxel list (line_claim_kernel: the one launch the storage unit asks for).  Asynchronous on `s`
int build_private_table(gp_voxelmap* m, hipStream_t s);
#pragma GCC visibility pop

}  // namespace gp
