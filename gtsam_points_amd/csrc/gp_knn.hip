// gp_knn.hip -- the structures of the exact k-nearest-neighbour search and its entry points: the build of the hashed and the binned grid (gp_knn_grid.hpp),
// gp_knn_search, the fused mean neighbour distance of the outlier filter, and the correspondence pass of the GICP / ICP / LOAM factors of gp_corr_factors.hip
// (BASELINE.json configs[4]).  The search itself is gp_knn_search.hpp; covariance and normal estimation are gp_covariance.hip.  The hashed grid's cell box and its
// key table are gp_cells.hpp's CellBox and gp_key_table.hpp's key_claim / key_find.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   ann/small_kdtree.hpp:124-186 (the tree build)                     KdTree                    -> gp_point_grid_create
//   ann/small_kdtree.hpp:437-474                                      knn_search                -> gp_knn_search
//   factors/impl/integrated_gicp_factor_impl.hpp:132-172              update_correspondences    -> gp::launch_nearest_correspondences
#include <algorithm>
#include <cstring>

#include "gp_host.hpp"
#include "gp_knn_search.hpp"
#include "gp_scan.hpp"

namespace gp {

// ---- grid build -------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) grid_insert_kernel(const float* __restrict__ points, int n, double inv_h, unsigned long long* __restrict__ keys,
                                                          int* __restrict__ counts, int* __restrict__ point_slot, uint32_t mask, int* __restrict__ bbox) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int j = i < n ? i : n - 1;  // the tail lanes repeat the last point so that the wave-wide min/max below needs no masking
  const int cx = hashed_cell((double)points[3 * (size_t)j] * inv_h), cy = hashed_cell((double)points[3 * (size_t)j + 1] * inv_h),
            cz = hashed_cell((double)points[3 * (size_t)j + 2] * inv_h);
  // bounding box of the occupied cells (bounds every query's cube radius): wave min/max, one row per workgroup, reduced by
  // bbox_reduce_kernel (atomics on six shared words serialise ~100 k operations per level: measured 1 ms)
  const int c[3] = {cx, cy, cz};
  CellBox box;
  box.add(c);
  __shared__ int wave_box[4][6];
  box.block_reduce(wave_box);
  if (threadIdx.x == 0) box.store(bbox + 6 * (size_t)blockIdx.x);
  if (i >= n) return;
  // the cell's slot (gp_key_table.hpp).  No room -- the probe came back to its home slot -- cannot happen at the load factor level_slots guarantees (<= 0.5); the
  // point would be left out of the grid (slot -1), the build cannot spin
  const unsigned long long key = pack_cell(cx, cy, cz);
  int claimed;
  const uint32_t s = key_claim(keys, mask, hash_key(key) & mask, key, &claimed);
  point_slot[i] = s <= mask ? (int)s : -1;
  if (s <= mask) atomicAdd(&counts[s], 1);
}

// per-workgroup boxes [nb][6] -> one box
__global__ void __launch_bounds__(256) bbox_reduce_kernel(const int* __restrict__ block_boxes, int nb, int* __restrict__ bbox) {
  CellBox box;
  for (int b = threadIdx.x; b < nb; b += 256) box.merge(block_boxes + 6 * (size_t)b);
  __shared__ int wave_box[4][6];
  box.block_reduce(wave_box);
  if (threadIdx.x == 0) box.store(bbox);
}

__global__ void __launch_bounds__(256) grid_scatter_kernel(const float* __restrict__ points, int n, const int* __restrict__ point_slot, const int* __restrict__ start,
                                                           int* __restrict__ cursor, float4* __restrict__ sorted) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int s = point_slot[i];
  if (s < 0) return;  // (a point grid_insert_kernel found no slot for)
  const int pos = start[s] + atomicAdd(&cursor[s], 1);
  sorted[pos] = make_float4(points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], __int_as_float(i));
}

// superblock occupancy: bit (bx & 3) + 4 (by & 3) + 16 (bz & 3) of entry (bx >> 2, by >> 2, bz >> 2), relative block coordinates
__global__ void super_mark_kernel(const int* __restrict__ occ_blocks, int num, GridGeom geom, int sdim0, int sdim1, unsigned long long* __restrict__ super,
                                  const FillJob caller_zero) {
  run_fill_job(caller_zero);  // (words the CALLER's kernels behind this one want zeroed: gp_estimate_covariances' counters)
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= num) return;
  const long long b = occ_blocks[i];
  const int bx = (int)(b % geom.dim[0]), by = (int)((b / geom.dim[0]) % geom.dim[1]), bz = (int)(b / ((long long)geom.dim[0] * geom.dim[1]));
  atomicOr(super + ((size_t)(bz >> 2) * sdim1 + (by >> 2)) * sdim0 + (bx >> 2), 1ull << ((bx & 3) | ((by & 3) << 2) | ((bz & 3) << 4)));
}

__global__ void __launch_bounds__(256) gather_sorted_kernel(const float* __restrict__ points, const int* __restrict__ order, int n, float4* __restrict__ sorted,
                                                           const FillJob zero_super) {
  run_fill_job(zero_super);  // (the superblock masks the kernel behind this one ORs into: gp_host.hpp, FillJob)
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= n) return;
  const size_t i = (size_t)order[j];
  sorted[j] = make_float4(points[3 * i], points[3 * i + 1], points[3 * i + 2], __int_as_float((int)i));
}

template <int KMAX>
__global__ void __launch_bounds__(128) knn_kernel(SearchView g, const float* __restrict__ queries, int nq, int k, double max_sq_dist, int* __restrict__ indices,
                                                  double* __restrict__ sq_dists, int* __restrict__ num_found) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= nq) return;
  TopK<KMAX> top;
  top.init(k, max_sq_dist);
  knn_query_any<KMAX>(g, (double)queries[3 * (size_t)i], (double)queries[3 * (size_t)i + 1], (double)queries[3 * (size_t)i + 2], 2 * k, top);
#pragma unroll
  for (int j = 0; j < KMAX; j++)
    if (j < k) {
      indices[(size_t)i * k + j] = j < top.found ? top.idx[j] : -1;
      if (sq_dists) sq_dists[(size_t)i * k + j] = top.d[j];
    }
  if (num_found) num_found[i] = top.found;
}

// find_inlier_points (point_cloud_cpu_funcs.cpp:576-600) without its neighbour lists: one query per lane as knn_kernel, but the list never leaves the registers --
// d_i = (sum_{j < k} sqrt(d2_j)) / k in list order (ascending distance; the point itself comes first with 0), 8 B per point stored instead of 12 k B.
// SHORT points -- a non-finite coordinate (no search is run for it) or fewer than k neighbours in the cloud -- store +inf and are counted.

template <int KMAX>
__global__ void __launch_bounds__(128) mean_neighbor_distance_kernel(SearchView g, const float* __restrict__ points, int n, int k, double* __restrict__ mean_dists,
                                                                     int* __restrict__ num_short) {
  const int i = blockIdx.x * 128 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  double mean = __longlong_as_double(0x7ff0000000000000ll);
  if (finite3(x, y, z)) {
    TopK<KMAX> top;
    top.init(k, 1.7976931348623157e308);
    knn_query_any<KMAX>(g, (double)x, (double)y, (double)z, 2 * k, top);
    if (top.found >= k) {
      double sum = 0.0;
#pragma unroll
      for (int j = 0; j < KMAX; j++)
        if (j < k) sum += sqrt(top.d[j]);
      mean = sum / (double)k;
    }
  }
  mean_dists[i] = mean;
  if (num_short && !(mean < 1.7976931348623157e308)) atomicAdd(num_short, 1);
}

// the same quantity from the caller's neighbour lists (the overload that takes them, :576-617): differences in f64 on the f32 coordinates, summed in list order.  An index
// outside [0, n) makes the point short and is never dereferenced; so does a non-finite coordinate of the point or of a listed neighbour.
__global__ void __launch_bounds__(256) mean_neighbor_distance_from_kernel(const float* __restrict__ points, int n, const int* __restrict__ neighbors, int k,
                                                                          double* __restrict__ mean_dists, int* __restrict__ num_short) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  const float x = points[3 * i], y = points[3 * i + 1], z = points[3 * i + 2];
  const double qx = (double)x, qy = (double)y, qz = (double)z;
  bool ok = finite3(x, y, z);
  double sum = 0.0;
  for (int j = 0; j < k && ok; j++) {
    const int nb = neighbors[i * (size_t)k + j];
    ok = nb >= 0 && nb < n;
    if (ok) {
      const float vx = points[3 * (size_t)nb], vy = points[3 * (size_t)nb + 1], vz = points[3 * (size_t)nb + 2];
      // the search's own expression.  That the two paths give the same bits rests on the compiler contracting it the same way in both kernels: not guaranteed by
      // construction (the search's kernels are left as they are), held by tests/test_outliers_gpu.py on every build
      const double ddx = (double)vx - qx, ddy = (double)vy - qy, ddz = (double)vz - qz;
      sum += sqrt(ddx * ddx + ddy * ddy + ddz * ddz);
    }
  }
  const double mean = sum / (double)k;
  ok = ok && mean < 1.7976931348623157e308;  // (false for inf and NaN)
  mean_dists[i] = ok ? mean : __longlong_as_double(0x7ff0000000000000ll);
  if (num_short && !ok) atomicAdd(num_short, 1);
}

// *num_short (when asked for) through a zeroed device counter behind the kernel: the one wait of gp_cloud_mean_neighbor_distances / _from
template <typename Launch>
int count_short_points(int* num_short, hipStream_t s, const Launch& launch) {
  if (!num_short) return launch(nullptr);
  DeviceArray counter;
  GP_TRY(counter.alloc_pooled(sizeof(int), s));
  GP_HIP(hipMemsetAsync(counter.ptr, 0, sizeof(int), s));
  GP_TRY(launch(counter.as<int>()));
  HostWords hw;
  GP_TRY(HostWords::get(&hw));
  GP_TRY(hw.finish(s, counter.as<int>(), 8));
  *num_short = reinterpret_cast<volatile int*>(hw.host)[8];
  counter.release_on(s);
  return GP_OK;
}

// ---- the correspondence pass of the matching-cost factors (gp_corr_factors.hip) ----------------------------------------------------
struct NearestDesc {
  const float* points;
  SearchView grid;
  int n;
  double max_sq_dist;
  double pose[16];  // rides in the kernel arguments (no H2D copy in front of the launch)
};

// update_correspondences of the GICP and ICP factors (integrated_gicp_factor_impl.hpp:132-172, integrated_icp_factor_impl.hpp:146-157):
// corr[i] = index of the nearest target point of T p_i with squared distance < max, or -1.  ONE query per lane and nothing else in
// the kernel: the search is a chain of dependent round trips that only occupancy hides, and a kernel that also held a factor's 32 f64
// accumulators and the algebra's temporaries next to the search state took 157 VGPRs (three waves per SIMD, and a 1 M-point cloud only brings 3.8).
// (92 VGPRs, five waves per SIMD.  Capped at 80 VGPRs -- six waves, eleven registers spilled -- it measured 2 % faster: not worth the scratch.)
__global__ void __launch_bounds__(256) nearest_correspond_kernel(NearestDesc f, int* __restrict__ corr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  const Pose Tl = load_pose(f.pose);
  const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
  const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
  const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
  const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
  TopK<1> top;
  top.init(1, f.max_sq_dist);
  knn_query_any<1>(f.grid, lx, ly, lz, 1, top);
  corr[i] = top.found ? top.idx[0] : -1;
}

// The same pass for a batch of factors (gp_corr_batch.hip) in ONE launch: the search structure, cloud and cut-off of factor t.factor come from a descriptor table and
// its pose from a pose table, both in device memory (the device-resident LM graph writes the poses there itself).  Four workgroups per tile of <= 1024 points, one
// query per lane as above; the query and the walk are the single launch's, so the correspondences are the same.
struct NearestBatchDesc {
  const float* points;
  SearchView grid;
  int* corr[2];  // the two correspondence sets
  int n;
  int k;  // neighbours kept per source point: 1 (GICP, ICP: nearest_correspond_batch_kernel) or 2 / 3 (LOAM edge / plane: nearest_k_correspond_batch_kernel)
  double max_sq_dist;
};

__global__ void __launch_bounds__(256) nearest_correspond_batch_kernel(const NearestBatchDesc* __restrict__ descs, const CorrTile* __restrict__ tiles,
                                                                       const double* __restrict__ poses, const int set) {
  const CorrTile t = tiles[blockIdx.x >> 2];
  const int k = (int)(blockIdx.x & 3) * 256 + (int)threadIdx.x;
  if (k >= t.count) return;
  const NearestBatchDesc& f = descs[t.factor];
  const int i = t.begin + k;
  const Pose Tl = load_pose(poses + 16 * (size_t)t.factor);
  const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
  const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
  const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
  const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
  TopK<1> top;
  top.init(1, f.max_sq_dist);
  knn_query_any<1>(f.grid, lx, ly, lz, 1, top);
  f.corr[set][i] = top.found ? top.idx[0] : -1;
}

// update_correspondences of the LOAM factors (integrated_loam_factor_impl.hpp:80-124 plane, K = 3; :235-279 edge, K = 2): the K nearest target points of T p_i with
// squared distance < max (the strict '<' of TopK::push) in ASCENDING order of distance -- index 0 is the anchor x_j of both residuals --, or -1 in every slot when
// fewer than K lie within the cut-off.  Stored as int[K][n] (corr[k * n + i]): lane i of a wave writes consecutive words of each of the K rows.  The list is FULL
// (k == KMAX): straight-line insertion, an entry is held iff its index is valid.  One query per lane and nothing else in the kernel, as above.
template <int K>
__device__ __forceinline__ void nearest_k_store(const SearchView& grid, const float* __restrict__ points, const Pose& Tl, double max_sq_dist, int i, int n,
                                                int* __restrict__ corr) {
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
  const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
  const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
  TopK<K, true> top;
  top.init(K, max_sq_dist);
  knn_query_any<K, true>(grid, lx, ly, lz, K, top);
  const bool all = top.idx[K - 1] >= 0;  // (the list is sorted: the last slot is filled last)
#pragma unroll
  for (int k = 0; k < K; k++) corr[(size_t)k * (size_t)n + (size_t)i] = all ? top.idx[k] : -1;
}

template <int K>
__global__ void __launch_bounds__(256) nearest_k_correspond_kernel(NearestDesc f, int* __restrict__ corr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  nearest_k_store<K>(f.grid, f.points, load_pose(f.pose), f.max_sq_dist, i, f.n, corr);
}

// ... and for the K > 1 members of a batch, in ONE launch over their tiles: search structure, cloud, cut-off and K from the descriptor table, the pose from the pose
// table, into the set it is given, as nearest_correspond_batch_kernel does for K = 1.  K is the same for the whole workgroup (a tile belongs to one factor).
__global__ void __launch_bounds__(256) nearest_k_correspond_batch_kernel(const NearestBatchDesc* __restrict__ descs, const CorrTile* __restrict__ tiles,
                                                                         const double* __restrict__ poses, const int set) {
  const CorrTile t = tiles[blockIdx.x >> 2];
  const int k = (int)(blockIdx.x & 3) * 256 + (int)threadIdx.x;
  if (k >= t.count) return;
  const NearestBatchDesc& f = descs[t.factor];
  const Pose Tl = load_pose(poses + 16 * (size_t)t.factor);
  if (f.k == 2)
    nearest_k_store<2>(f.grid, f.points, Tl, f.max_sq_dist, t.begin + k, f.n, f.corr[set]);
  else
    nearest_k_store<3>(f.grid, f.points, Tl, f.max_sq_dist, t.begin + k, f.n, f.corr[set]);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

namespace gp {
// the one thing the matching-cost factors need of the search (declared in gp_host.hpp; n > 0)
int launch_nearest_correspondences(const gp_point_grid* grid, const float* points, int n, const double pose_lin[16], double max_sq_dist, int* corr, hipStream_t stream) {
  NearestDesc f;
  f.points = points;
  f.grid = grid->view();  // the max-distance bound terminates the search early (worst() starts at max_sq_dist)
  f.n = n;
  f.max_sq_dist = max_sq_dist;
  memcpy(f.pose, pose_lin, sizeof(double) * 16);
  hipLaunchKernelGGL(nearest_correspond_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, f, corr);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int launch_nearest_k_correspondences(const gp_point_grid* grid, const float* points, int n, int k, const double pose_lin[16], double max_sq_dist, int* corr, hipStream_t stream) {
  if (k != 2 && k != 3) return fail(GP_ERROR_INVALID_ARGUMENT, "launch_nearest_k_correspondences: k must be 2 or 3");
  NearestDesc f;
  f.points = points;
  f.grid = grid->view();
  f.n = n;
  f.max_sq_dist = max_sq_dist;
  memcpy(f.pose, pose_lin, sizeof(double) * 16);
  if (k == 2)
    hipLaunchKernelGGL(nearest_k_correspond_kernel<2>, dim3((n + 255) / 256), dim3(256), 0, stream, f, corr);
  else
    hipLaunchKernelGGL(nearest_k_correspond_kernel<3>, dim3((n + 255) / 256), dim3(256), 0, stream, f, corr);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

size_t corr_search_desc_bytes() { return sizeof(NearestBatchDesc); }

void fill_corr_search_desc(void* table_host, int index, const gp_point_grid* grid, const float* points, int n, double max_sq_dist, int* corr0, int* corr1, int k) {
  NearestBatchDesc d{};
  d.points = points;
  d.grid = grid->view();
  d.corr[0] = corr0, d.corr[1] = corr1;
  d.n = n;
  d.k = k;
  d.max_sq_dist = max_sq_dist;
  memcpy(static_cast<char*>(table_host) + sizeof(NearestBatchDesc) * (size_t)index, &d, sizeof(d));
}

int launch_nearest_correspondences_batch(const void* table_dev, const CorrTile* tiles_dev, int num_tiles, const double* poses_dev, int set, hipStream_t stream) {
  hipLaunchKernelGGL(nearest_correspond_batch_kernel, dim3(4 * (unsigned)num_tiles), dim3(256), 0, stream, static_cast<const NearestBatchDesc*>(table_dev), tiles_dev, poses_dev, set);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int launch_nearest_k_correspondences_batch(const void* table_dev, const CorrTile* tiles_dev, int num_tiles, const double* poses_dev, int set, hipStream_t stream) {
  hipLaunchKernelGGL(nearest_k_correspond_batch_kernel, dim3(4 * (unsigned)num_tiles), dim3(256), 0, stream, static_cast<const NearestBatchDesc*>(table_dev), tiles_dev, poses_dev, set);
  GP_HIP(hipGetLastError());
  return GP_OK;
}
}  // namespace gp

extern "C" {

static inline size_t align256(size_t b) { return (b + 255) & ~size_t(255); }

static uint32_t level_slots(int n) {
  uint32_t slots = 1024;
  while (slots < 2u * (uint32_t)std::max(n, 1)) slots <<= 1;  // at most n distinct cells -> load factor <= 0.5
  return slots;
}

// scratch of one level build (counts | cursor | point_slot | block_sums | bbox), reused by every level of a grid
static size_t level_scratch_bytes(int n) {
  const uint32_t slots = level_slots(n);
  const size_t nb = (slots + gp::kScanThreads - 1) / gp::kScanThreads;
  return 2 * align256(sizeof(int) * slots) + align256(sizeof(int) * (size_t)std::max(n, 1)) + align256(sizeof(int) * nb) +
         align256(sizeof(int) * 6 * (((size_t)std::max(n, 1) + 255) / 256));
}

static int build_level(const float* points_dev, int n, double cell_size, hipStream_t s, char* scratch, int* bbox, gp_grid_level** out) {
  auto* g = new gp_grid_level;
  g->n = n;
  g->h = cell_size;
  const uint32_t slots = level_slots(n);
  g->mask = slots - 1;
  const int nb = (int)((slots + gp::kScanThreads - 1) / gp::kScanThreads);
  const size_t keys_b = align256(sizeof(unsigned long long) * slots), start_b = align256(sizeof(int) * ((size_t)slots + 1)),
               sorted_b = align256(sizeof(float4) * (size_t)std::max(n, 1));
  const int rc = g->arena.alloc_async(keys_b + start_b + sorted_b, s);
  if (rc != GP_OK) {
    delete g;
    return rc;
  }
  g->keys_p = g->arena.as<char>();
  g->start_p = g->arena.as<char>() + keys_b;
  g->sorted_p = g->arena.as<char>() + keys_b + start_b;
  unsigned long long* keys = static_cast<unsigned long long*>(g->keys_p);
  int* start = static_cast<int*>(g->start_p);
  float4* sorted = static_cast<float4*>(g->sorted_p);
  char* cur = scratch;
  int* counts = reinterpret_cast<int*>(cur);
  cur += align256(sizeof(int) * slots);
  int* cursor = reinterpret_cast<int*>(cur);
  cur += align256(sizeof(int) * slots);
  int* point_slot = reinterpret_cast<int*>(cur);
  cur += align256(sizeof(int) * (size_t)std::max(n, 1));
  int* block_sums = reinterpret_cast<int*>(cur);
  cur += align256(sizeof(int) * (size_t)nb);
  int* block_boxes = reinterpret_cast<int*>(cur);
  GP_HIP(hipMemsetAsync(keys, 0xff, sizeof(unsigned long long) * slots, s));
  GP_HIP(hipMemsetAsync(counts, 0, 2 * align256(sizeof(int) * slots), s));  // counts and cursor are adjacent
  if (n > 0) {
    const int blocks = (n + 255) / 256;
    hipLaunchKernelGGL(gp::grid_insert_kernel, dim3(blocks), dim3(256), 0, s, points_dev, n, 1.0 / cell_size, keys, counts, point_slot, g->mask, block_boxes);
    hipLaunchKernelGGL(gp::bbox_reduce_kernel, dim3(1), dim3(256), 0, s, block_boxes, blocks, bbox);
  }
  // exclusive scan of counts[0..slots) -> start[0..slots], three small kernels (block sums, scan of block sums, add); the grand total goes straight to start[slots]
  hipLaunchKernelGGL(gp::strided_scan_block_kernel<0>, dim3(nb), dim3(gp::kScanThreads), 0, s, (const int*)counts, 1, start, 1, block_sums, (long long)slots);
  hipLaunchKernelGGL(gp::strided_scan_sums_kernel<0>, dim3(1), dim3(gp::kScanThreads), 0, s, block_sums, nb, start + slots);
  hipLaunchKernelGGL(gp::strided_scan_add_kernel<0>, dim3(nb), dim3(gp::kScanThreads), 0, s, start, 1, (const int*)block_sums, (long long)slots);
  if (n > 0) {
    hipLaunchKernelGGL(gp::grid_scatter_kernel, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, n, point_slot, start, cursor, sorted);
  }
  GP_HIP(hipGetLastError());
  // no synchronisation here: the next level reuses the scratch in stream order; the caller fetches all bounding boxes at once
  *out = g;
  return GP_OK;
}

// levels: cell_size, 4 cell_size, 16 cell_size (coarser levels only when the cloud is large enough to need them)
int gp_point_grid_create(const float* points_dev, int n, double cell_size, gp_stream_t stream, gp_point_grid_t** out) {
  return gp_point_grid_create_ex(points_dev, n, cell_size, 0, nullptr, stream, out);
}

// structure: GP_TUNE_KNN_STRUCTURE value (0 binned + per-lane search, 1 hashed multi-level grid, 3 row-tiled covariance pass first, 4 two binned
// levels); counters_dev: device buffer of 8 uint64 work counters (measurement) or null
int gp_point_grid_create_ex(const float* points_dev, int n, double cell_size, int structure, unsigned long long* counters_dev, gp_stream_t stream, gp_point_grid_t** out) {
  // (synchronised: gp_knn_search takes a stream of its own, which need not be the one the structure was built on)
  return gp::point_grid_create_impl(points_dev, n, cell_size, structure, counters_dev, stream, false, true, out);
}

}  // extern "C"

namespace gp {
int point_grid_create_impl(const float* points_dev, int n, double cell_size, int structure, unsigned long long* counters_dev, gp_stream_t stream, bool keep_cell_of,
                           bool synchronise, gp_point_grid_t** out, const FillJob caller_zero, bool* caller_zero_applied) {
  bool caller_zero_done = false;
  struct Report {
    bool* out;
    const bool* done;
    ~Report() {
      if (out) *out = *done;
    }
  } report{caller_zero_applied, &caller_zero_done};
  if (!points_dev || n < 0 || !(cell_size > 0.0) || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_point_grid_create: bad arguments");
  if (structure != 0 && structure != 1 && structure != 3 && structure != 4 && structure != 6 && structure != 7 && structure < 16)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_point_grid_create_ex: structure in {0, 1, 3, 4, 6, 7} (>= 16: staging experiment)");
  auto* g = new gp_point_grid;
  g->stream = (hipStream_t)stream;
  g->structure = structure;
  g->counters = counters_dev;
  const bool force_hashed_grid = structure == 1;
  const int knn_levels = structure == 4 ? 2 : 1;  // binned levels (cell size x4 each); the blocks of the last one serve as the coarse level
  if (n > 0 && !force_hashed_grid) {
    // binned levels h, 4h, 16h (one level for small clouds and for radius-bounded searches, which never leave the first shells)
    const int want_levels = (n > 4096 && knn_levels > 1) ? std::min(knn_levels, gp::kMaxLevels) : 1;
    int rc = GP_OK;
    bool ok = true;
    double h = cell_size;
    for (int l = 0; l < want_levels && ok && rc == GP_OK; l++, h *= 4.0) {
      auto lv = std::make_unique<gp_point_grid::BinLevel>();
      bool too_large = false;
      rc = gp::bin_points(points_dev, n, 1.0 / h, g->stream, &lv->bins, &too_large);
      if (rc != GP_OK) break;
      if (too_large || lv->bins.num_cells <= 0) {
        ok = false;
        break;
      }
      rc = lv->sorted.alloc_pooled(sizeof(float4) * (size_t)std::max(lv->bins.num_binned, 1), g->stream);
      if (rc != GP_OK) break;
      // superblock occupancy (coarse stage of the search): zeroed by the gather kernel on its way, marked by the kernel behind it
      size_t sn = 1;
      for (int a = 0; a < 3; a++) {
        lv->sdim[a] = (lv->bins.geom.dim[a] + 3) / 4;
        sn *= (size_t)lv->sdim[a];
      }
      const size_t super_bytes = (sizeof(unsigned long long) * sn + 255) & ~size_t(255);
      rc = lv->super.alloc_pooled(super_bytes, g->stream);
      if (rc != GP_OK) break;
      hipLaunchKernelGGL(gp::gather_sorted_kernel, dim3((std::max(lv->bins.num_binned, 1) + 255) / 256), dim3(256), 0, g->stream, points_dev, (const int*)lv->bins.order.as<int>(),
                         lv->bins.num_binned, lv->sorted.as<float4>(), gp::fill_job(lv->super.ptr, super_bytes, 0u));
      // (launched also without occupied blocks when it carries the caller's fill)
      if (lv->bins.num_occ_blocks > 0 || (l == 0 && caller_zero.count > 0))
        hipLaunchKernelGGL(gp::super_mark_kernel, dim3((std::max(lv->bins.num_occ_blocks, 1) + 255) / 256), dim3(256), 0, g->stream, (const int*)lv->bins.occ_blocks.as<int>(),
                           lv->bins.num_occ_blocks, lv->bins.geom, lv->sdim[0], lv->sdim[1], lv->super.as<unsigned long long>(), l == 0 ? caller_zero : gp::FillJob{});
      if (l == 0) caller_zero_done = true;
      {
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) rc = gp::hip_fail(e, "gather_sorted_kernel", __FILE__, __LINE__);
      }
      if (synchronise && rc == GP_OK) {
        const hipError_t e = hipStreamSynchronize(g->stream);
        if (e != hipSuccess) rc = gp::hip_fail(e, "gather_sorted_kernel", __FILE__, __LINE__);
      }
      // (the arrays below go back to the pool in stream order)
      lv->h = h;
      lv->bins.order.release_on(g->stream);  // only the sorted copy is searched
      if (!(keep_cell_of && l == 0)) lv->bins.cell_of.release_on(g->stream);
      lv->bins.cell_block.release_on(g->stream);
      g->bin_levels.push_back(std::move(lv));
    }
    if (rc != GP_OK) {
      delete g;
      return rc;
    }
    if (ok && !g->bin_levels.empty()) {
      g->binned = true;
      g->num_binned = g->bin_levels[0]->bins.num_binned;
      *out = g;
      return GP_OK;
    }
    g->bin_levels.clear();  // bounding box too large for the block grid: hashed fallback below
  }
  const int num_levels = n > 4096 ? gp::kMaxLevels : 1;
  gp::DeviceArray scratch;
  {
    const int rc = scratch.alloc_async(level_scratch_bytes(n), g->stream);
    if (rc != GP_OK) {
      delete g;
      return rc;
    }
  }
  gp::DeviceArray d_bbox;
  int h_bbox[6 * gp::kMaxLevels];
  {
    const int rc = d_bbox.alloc_async(sizeof(int) * 6 * gp::kMaxLevels, g->stream);
    if (rc != GP_OK) {
      delete g;
      return rc;
    }
  }
  double h = cell_size;
  for (int l = 0; l < num_levels; l++, h *= 4.0) {
    gp_grid_level* lv = nullptr;
    const int rc = build_level(points_dev, n, h, g->stream, scratch.as<char>(), d_bbox.as<int>() + 6 * l, &lv);
    if (rc != GP_OK) {
      delete g;
      return rc;
    }
    g->levels.emplace_back(lv);
  }
  // one copy + one synchronisation for the whole structure (the scratch and d_bbox go back to the pool on return)
  hipError_t e = hipMemcpyAsync(h_bbox, d_bbox.ptr, sizeof(int) * 6 * (size_t)num_levels, hipMemcpyDeviceToHost, g->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(g->stream);
  if (e != hipSuccess) {
    delete g;
    return gp::hip_fail(e, "gp_point_grid_create", __FILE__, __LINE__);
  }
  if (n > 0) {
    const int* hb = h_bbox;
    for (int l = 0; l < num_levels; l++)
      for (int a = 0; a < 3; a++) {
        g->levels[l]->lo[a] = hb[6 * l + a];
        g->levels[l]->hi[a] = hb[6 * l + 3 + a];
      }
  }
  *out = g;
  return GP_OK;
}
}  // namespace gp

extern "C" {

int gp_point_grid_destroy(gp_point_grid_t* g) {
  if (!g) return GP_OK;
  // the arenas come from the stream-ordered pool and are returned to it in the order of the creation stream: searches issued
  // on other streams must have finished first (hipFree used to imply this)
  (void)hipDeviceSynchronize();
  delete g;
  return GP_OK;
}

int gp_knn_search(const gp_point_grid_t* g, const float* queries_dev, int nq, int k, double max_sq_dist, int* indices_dev, double* sq_dists_dev, int* num_found_dev,
                  gp_stream_t stream) {
  if (!g || !queries_dev || nq < 0 || k <= 0 || k > 32 || !indices_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_knn_search: bad arguments (1 <= k <= 32)");
  if (nq == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  const gp::SearchView v = g->view();
  const dim3 grid((nq + 127) / 128), block(128);
  if (k == 1)
    hipLaunchKernelGGL(gp::knn_kernel<1>, grid, block, 0, s, v, queries_dev, nq, k, max_sq_dist, indices_dev, sq_dists_dev, num_found_dev);
  else if (k <= 10)
    hipLaunchKernelGGL(gp::knn_kernel<10>, grid, block, 0, s, v, queries_dev, nq, k, max_sq_dist, indices_dev, sq_dists_dev, num_found_dev);
  else
    hipLaunchKernelGGL(gp::knn_kernel<32>, grid, block, 0, s, v, queries_dev, nq, k, max_sq_dist, indices_dev, sq_dists_dev, num_found_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_cloud_mean_neighbor_distances(const gp_point_grid_t* g, const float* points_dev, int n, int k, double* mean_dists_dev, int* num_short, gp_stream_t stream) {
  if (n < 0 || k < 1 || k > 32) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_mean_neighbor_distances: bad arguments (n >= 0, 1 <= k <= 32)");
  if (n > 0 && (!g || !points_dev || !mean_dists_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_mean_neighbor_distances: NULL grid / array");
  if (num_short) *num_short = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  const gp::SearchView v = g->view();
  const dim3 grid((n + 127) / 128), block(128);
  return gp::count_short_points(num_short, s, [&](int* counter) {
    if (k == 1)
      hipLaunchKernelGGL(gp::mean_neighbor_distance_kernel<1>, grid, block, 0, s, v, points_dev, n, k, mean_dists_dev, counter);
    else if (k <= 10)
      hipLaunchKernelGGL(gp::mean_neighbor_distance_kernel<10>, grid, block, 0, s, v, points_dev, n, k, mean_dists_dev, counter);
    else
      hipLaunchKernelGGL(gp::mean_neighbor_distance_kernel<32>, grid, block, 0, s, v, points_dev, n, k, mean_dists_dev, counter);
    GP_HIP(hipGetLastError());
    return (int)GP_OK;
  });
}

int gp_cloud_mean_neighbor_distances_from(const float* points_dev, int n, const int* neighbors_dev, int k, double* mean_dists_dev, int* num_short, gp_stream_t stream) {
  if (n < 0 || k < 1) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_mean_neighbor_distances_from: bad arguments (n >= 0, k >= 1)");
  if (n > 0 && (!points_dev || !neighbors_dev || !mean_dists_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_mean_neighbor_distances_from: NULL array");
  if (num_short) *num_short = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  return gp::count_short_points(num_short, s, [&](int* counter) {
    hipLaunchKernelGGL(gp::mean_neighbor_distance_from_kernel, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, n, neighbors_dev, k, mean_dists_dev, counter);
    GP_HIP(hipGetLastError());
    return (int)GP_OK;
  });
}

}  // extern "C"
