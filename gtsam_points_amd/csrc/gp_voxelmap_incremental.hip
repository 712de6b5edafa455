// gp_voxelmap_incremental.hip -- the incremental insert of the Gaussian voxel map with LRU eviction: the sliding local map of scan-to-model odometry.
//
// The reference's GPU map cannot do this ("Incremental insertion is not supported for GPU", types/gaussian_voxelmap_gpu.hpp:63); its CPU map can: GaussianVoxelMapCPU
// is an IncrementalVoxelMap<GaussianVoxel> (gaussian_voxelmap_cpu.cpp:23-47, ann/impl/incremental_voxelmap_impl.hpp:31-68), and this unit restates THAT insert:
//   1. every finite, in-range point goes to the voxel fast_floor(p / leaf), created empty when absent: count += 1, sums += point and covariance,
//      intensity = max(intensity, I), stamp = lru_counter; a voxel the frame does not touch keeps everything
//   2. ++lru_counter; when lru_counter % lru_clear_cycle == 0 every voxel with stamp + lru_horizon < lru_counter goes (with lru_horizon = 0 the ones just touched too)
//   3. mean = sum / count, cov = sum(cov) / count
// as a VOXEL-LEVEL MERGE, O(old voxels + new points + blocks), with no per-point atomics.  The unit holds the three kernels that only it launches (below); the bounding
// box, the block grid and the bucket placement are gp_voxelmap.hip's, through the helpers of gp_voxelmap.hpp:
//   bin_points + segmented_sums_kernel   the frame's distinct cells with their counts, f64 sums and intensities -- the binned build's lanes and summation order
//   the union box                        of the surviving old voxels (the old grid's box; on a clearing call the box of the survivors, so that the grid follows the
//                                        sliding map instead of growing along the whole trajectory) and of the frame's cells.  A box beyond kMaxGridBlocks is REFUSED
//                                        (GP_ERROR_INVALID_ARGUMENT, map and counter untouched): a hashed fallback like the one-shot build's is not built here
//   a fresh block grid (build_block_grid) bits from the survivors and the cells, counts, exclusive scan: the merged map's numbering is (block, bit) order
//   merge_source / merge_finalize        per merged voxel at most one old voxel and one cell: old + new in f64, then everything the map keeps of a voxel
//   place_voxels                         the reference-visible bucket table, along the binned build's doubling sequence
// The sums are kept per voxel in f64 (gp_voxelmap::kSums) beside the stamps (kStamps); the f32 mean_local of the gather record is rounded from them once per insert,
// so the rounding does not compound.  The new arrays are swapped in only when all of this has succeeded.
// A map that holds voxels but no sums (built by insert, assign or load) is refused, not adopted.
#include "gp_scan.hpp"
#include "gp_voxelmap.hpp"
#include "gp_voxelmap_kernels.hpp"

namespace gp {

// The frame is binned like a one-shot build's cloud; segmented_sums_kernel leaves each of its cells' count, f64 sums, intensity and coordinate.  The surviving old
// voxels and the new cells mark their bits in a FRESH block grid over the union box; a voxel of the merged map is a set bit, numbered in (block, bit) order like
// every map.  merge_source_kernel writes, per merged voxel, which old voxel and which new cell it is made of (-1: none); merge_finalize_kernel gathers the two, adds
// old + new in f64 and emits everything the map keeps of a voxel.  No atomics on sums: two maps fed the same frames hold the same bits.

// a source of the merge as merge_finalize_kernel gathers it: the old map's per-voxel arrays, or the frame's per-cell arrays (stamps == null)
struct MergeSource {
  const int* coords;
  const int* counts;
  const double* sums;
  const float* intensities;
  const long long* stamps;
};

// the sums of the frame's cells, as segmented_stats_kernel forms them (same lanes, same order), not finalized
__global__ void __launch_bounds__(256) segmented_sums_kernel(const float* __restrict__ points, const float* __restrict__ covs, const float* __restrict__ intensities,
                                                             int num_cells, const int* __restrict__ cell_start, const int* __restrict__ order, double inv_leaf, double leaf,
                                                             int* __restrict__ cell_counts, double* __restrict__ cell_sums, float* __restrict__ cell_intensities,
                                                             int* __restrict__ cell_coords) {
  SegmentSums sum;
  if (!segmented_sums(points, covs, intensities, num_cells, cell_start, order, inv_leaf, leaf, sum)) return;
  const size_t c = (size_t)sum.v;
  cell_counts[c] = sum.n;
#pragma unroll
  for (int k = 0; k < 9; k++) cell_sums[9 * c + k] = sum.acc[k];
  cell_intensities[c] = sum.imax;
  cell_coords[3 * c] = sum.cx;
  cell_coords[3 * c + 1] = sum.cy;
  cell_coords[3 * c + 2] = sum.cz;
}

// source[new index] = v for every old voxel (or new cell) v whose bit is set in the new grid.  For an old voxel that is: it survived by its stamp, or the frame
// touches it (the cell set the bit) -- exactly the voxels the reference keeps, whose stamp of a touched voxel is the current counter.  An evicted voxel may lie
// outside the new box
__global__ void __launch_bounds__(256) merge_source_kernel(int num, const int* __restrict__ coords, GridGeom g, const GridBlock* __restrict__ blocks,
                                                           int* __restrict__ source) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num) return;
  const int cx = coords[3 * (size_t)v], cy = coords[3 * (size_t)v + 1], cz = coords[3 * (size_t)v + 2];
  if (!grid_contains(g, cx, cy, cz)) return;
  const int nv = grid_ordinal(g, blocks, cx, cy, cz);
  if (nv >= 0) source[nv] = v;
}

// one thread per voxel of the merged map: old + new in f64 (a voxel of one source alone keeps that source's sums to the bit), then the one-shot build's emit
__global__ void __launch_bounds__(256) merge_finalize_kernel(int num_voxels, const int* __restrict__ source_old, const int* __restrict__ source_new, MergeSource old,
                                                             MergeSource cell, long long stamp_now, double leaf, double* __restrict__ sums,
                                                             long long* __restrict__ stamps, VoxelOutputs out, const gp::FillJob fill_buckets) {
  gp::run_fill_job(fill_buckets);  // (the bucket table insert_voxels_kernel claims its slots in behind this kernel: 0xff = empty)
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int so = source_old[v], sn = source_new[v];  // at least one of the two is a source: the bit was set by one of them
  double acc[9];
  int n = 0, cx = 0, cy = 0, cz = 0;
  float imax = 0.0f;
  long long stamp = stamp_now;
  if (so >= 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) acc[k] = old.sums[9 * (size_t)so + k];
    n = old.counts[so];
    imax = old.intensities[so];
    stamp = old.stamps[so];
    cx = old.coords[3 * (size_t)so], cy = old.coords[3 * (size_t)so + 1], cz = old.coords[3 * (size_t)so + 2];
  }
  if (sn >= 0) {
#pragma unroll
    for (int k = 0; k < 9; k++) {
      const double x = cell.sums[9 * (size_t)sn + k];
      acc[k] = so >= 0 ? acc[k] + x : x;
    }
    n += cell.counts[sn];
    imax = intensity_max(imax, cell.intensities[sn]);
    stamp = stamp_now;
    cx = cell.coords[3 * (size_t)sn], cy = cell.coords[3 * (size_t)sn + 1], cz = cell.coords[3 * (size_t)sn + 2];
  }
  if (so < 0 && sn < 0) return;  // (cannot happen; nothing is written from undefined sums)
#pragma unroll
  for (int k = 0; k < 9; k++) sums[9 * (size_t)v + k] = acc[k];
  stamps[v] = stamp;
  emit_voxel(out, v, n, acc, imax, cx, cy, cz, voxel_centre(cx, leaf), voxel_centre(cy, leaf), voxel_centre(cz, leaf));
}

}  // namespace gp

namespace {

// the device is idle on `s` before the scratch of a failed insert goes back to the pool (declared behind the arrays it guards)
struct DrainOnFailure {
  hipStream_t s;
  bool armed = true;
  ~DrainOnFailure() {
    if (armed) (void)hipStreamSynchronize(s);
  }
};

void join_box(int box[6], const gp::GridGeom& g) {
  for (int a = 0; a < 3; a++) {
    box[a] = std::min(box[a], g.lo[a]);
    box[3 + a] = std::max(box[3 + a], g.lo[a] + g.dim[a] - 1);
  }
}

int refuse_box() {
  return gp::fail(GP_ERROR_INVALID_ARGUMENT,
                  "gp_voxelmap_insert_incremental: the box of the map's voxels and the frame exceeds the block grid (2^24 blocks of 4 x 4 x 4 voxels); the map is unchanged");
}

}  // namespace

extern "C" {

int gp_voxelmap_insert_incremental(gp_voxelmap_t* m, const float* points_dev, const float* covs_dev, const float* intensities_dev, int n) {
  if (!m) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_insert_incremental: null map");
  if (n < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_insert_incremental: negative size");
  if (n > 0 && (!points_dev || !covs_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "error: GPU points/covs not allocated!!");
  if (m->offloaded) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_insert_incremental: voxel map is not on the GPU");
  if (m->info.num_voxels > 0 && !m->has_sums)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT,
                    "gp_voxelmap_insert_incremental: the map was built by insert, assign or load and holds no sums; an incremental map starts empty");
  hipStream_t s = m->stream;
  const int V_old = m->has_sums ? m->info.num_voxels : 0;
  const long long stamp_now = m->lru_counter, counter = stamp_now + 1;
  const int evict = counter % m->lru_clear_cycle == 0;
  const long long horizon = m->lru_horizon;
  const bool keep_nothing = evict && horizon == 0;  // every stamp is <= stamp_now < counter: the voxels just touched go too, as upstream

  gp::PointBins bins;
  gp::DeviceArray cell_counts, cell_sums, cell_intensities, cell_coords, box_dev, scratch, source_old, source_new, blocks;
  gp_voxelmap::Array fresh[gp_voxelmap::kGblocks];  // the merged map's rows of the table (kGblocks: `blocks`)
  DrainOnFailure drain{s};

  // ---- the frame's cells ----
  int C = 0;
  if (n > 0) {
    bool too_large = false;
    GP_TRY(gp::bin_points(points_dev, n, 1.0 / m->resolution, s, &bins, &too_large));
    if (too_large) return refuse_box();
    C = bins.num_cells;
  }
  if (keep_nothing) C = 0;
  const bool old_live = V_old > 0 && !keep_nothing;

  // ---- the union box, in block units ----
  int box[6];
  gp::empty_bbox(box);
  if (old_live && !evict) join_box(box, m->grid);  // (a map with voxels and sums was built here: it has its grid)
  const gp::VoxelSet old_voxels{old_live ? V_old : 0, m->voxel_coords.as<int>(), m->voxel_stamps.as<long long>(), evict, horizon, counter};
  if (old_live && evict) {
    GP_TRY(box_dev.alloc_async(sizeof(box), s));
    GP_TRY(gp::voxels_bbox(old_voxels, box_dev.as<int>(), box, s));
  }
  if (C > 0) join_box(box, bins.geom);
  const bool any = box[0] <= box[3];
  gp::GridGeom g{};
  long long nb = 0;
  if (any && !gp::grid_geometry(box, &g, &nb)) return refuse_box();

  int V = 0;
  if (any) {
    // ---- the frame's sums per cell ----
    if (C > 0) {
      GP_TRY(cell_counts.alloc_async(sizeof(int) * (size_t)C, s));
      GP_TRY(cell_sums.alloc_async(sizeof(double) * 9 * (size_t)C, s));
      GP_TRY(cell_intensities.alloc_async(sizeof(float) * (size_t)C, s));
      GP_TRY(cell_coords.alloc_async(sizeof(int) * 3 * (size_t)C, s));
      hipLaunchKernelGGL(gp::segmented_sums_kernel, dim3((C + 15) / 16), dim3(256), 0, s, points_dev, covs_dev, intensities_dev, C, (const int*)bins.cell_start.as<int>(),
                         (const int*)bins.order.as<int>(), 1.0 / m->resolution, m->resolution, cell_counts.as<int>(), cell_sums.as<double>(), cell_intensities.as<float>(),
                         cell_coords.as<int>());
      GP_HIP(hipGetLastError());
    }
    // ---- a fresh block grid over the union box: bits of the survivors and of the cells, counts, scan ----
    GP_TRY(blocks.alloc_pooled(sizeof(gp::GridBlock) * (size_t)nb, s));
    GP_TRY(scratch.alloc_async(sizeof(int) * gp::scan_scratch_ints(nb), s));
    const gp::VoxelSet sets[2] = {old_voxels, {C, cell_coords.as<int>(), nullptr, 0, 0, 0}};
    GP_TRY(gp::build_block_grid(g, nb, blocks.as<gp::GridBlock>(), scratch.as<int>(), sets, 2, s));
    // (the scan leaves its grand total, the merged map's voxel count, behind its block sums: gp_scan.hpp)
    gp::HostWords hw;
    GP_TRY(gp::HostWords::get(&hw));
    GP_TRY(hw.finish(s, scratch.as<int>() + (nb + gp::kScanThreads - 1) / gp::kScanThreads, 13));
    V = reinterpret_cast<volatile int*>(hw.host)[13];
    if (V <= 0 || V > V_old + C) return gp::fail(GP_ERROR_HIP, "gp_voxelmap_insert_incremental: the merged grid holds an impossible number of voxels");
  }

  // ---- the merged map's arrays ----
  const size_t Vz = (size_t)V;
  GP_TRY(fresh[gp_voxelmap::kRecords].dev.alloc_pooled(sizeof(gp::VoxelRecord) * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kNumPoints].dev.alloc_pooled(sizeof(int) * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kMeans].dev.alloc_pooled(sizeof(float) * 3 * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kCovs].dev.alloc_pooled(sizeof(float) * 9 * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kIntensities].dev.alloc_pooled(sizeof(float) * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kCoords].dev.alloc_pooled(sizeof(int) * 3 * std::max<size_t>(Vz, 1), s));
  GP_TRY(fresh[gp_voxelmap::kSums].dev.alloc_pooled(sizeof(double) * 9 * Vz, s));
  GP_TRY(fresh[gp_voxelmap::kStamps].dev.alloc_pooled(sizeof(long long) * Vz, s));
  // the bucket table enters the doubling sequence where the binned build does; its first table is filled with "empty" by merge_finalize_kernel on its way
  int64_t num_buckets = gp::entry_bucket_count(m->init_num_buckets, m->bucket_load_percent, V);
  if (num_buckets > gp::kMaxBuckets) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_insert_incremental: bucket table would exceed 2^30 entries");
  gp::DeviceArray& buckets = fresh[gp_voxelmap::kBuckets].dev;
  GP_TRY(buckets.alloc_pooled(sizeof(gp_voxel_bucket) * (size_t)num_buckets, s));
  const gp::VoxelOutputs out = gp::voxel_outputs(fresh);
  if (V > 0) {
    GP_TRY(source_old.alloc_async(sizeof(int) * Vz, s));
    GP_TRY(source_new.alloc_async(sizeof(int) * Vz, s));
    GP_HIP(hipMemsetAsync(source_old.ptr, 0xff, sizeof(int) * Vz, s));
    GP_HIP(hipMemsetAsync(source_new.ptr, 0xff, sizeof(int) * Vz, s));
    const gp::MergeSource old{m->voxel_coords.as<int>(), m->num_points.as<int>(), m->voxel_sums.as<double>(), m->voxel_intensities.as<float>(), m->voxel_stamps.as<long long>()};
    const gp::MergeSource cell{cell_coords.as<int>(), cell_counts.as<int>(), cell_sums.as<double>(), cell_intensities.as<float>(), nullptr};
    if (old_live) {
      hipLaunchKernelGGL(gp::merge_source_kernel, dim3(gp::blocks_of(V_old)), dim3(256), 0, s, V_old, old.coords, g, (const gp::GridBlock*)blocks.as<gp::GridBlock>(),
                         source_old.as<int>());
      GP_HIP(hipGetLastError());
    }
    if (C > 0) {
      hipLaunchKernelGGL(gp::merge_source_kernel, dim3(gp::blocks_of(C)), dim3(256), 0, s, C, cell.coords, g, (const gp::GridBlock*)blocks.as<gp::GridBlock>(),
                         source_new.as<int>());
      GP_HIP(hipGetLastError());
    }
    hipLaunchKernelGGL(gp::merge_finalize_kernel, dim3(gp::blocks_of(Vz)), dim3(256), 0, s, V, (const int*)source_old.as<int>(), (const int*)source_new.as<int>(), old, cell,
                       stamp_now, m->resolution, fresh[gp_voxelmap::kSums].dev.as<double>(), fresh[gp_voxelmap::kStamps].dev.as<long long>(), out,
                       gp::fill_job(buckets.ptr, sizeof(gp_voxel_bucket) * (size_t)num_buckets, 0xffffffffu));
    GP_HIP(hipGetLastError());
  }
  // `buckets` and the count stay local until everything has succeeded: the map is untouched otherwise
  GP_TRY(gp::place_voxels("gp_voxelmap_insert_incremental", out.coords, out.num_points, V, buckets, &num_buckets, m->info.max_bucket_scan_count, V > 0, s));
  GP_HIP(hipStreamSynchronize(s));  // (the flag says the results are there; the old arrays and the scratch go back to the pool behind the kernels themselves)
  drain.armed = false;

  // ---- success: the merged map replaces the old one ----
  // the old arrays go back to the block cache ("any stream may take them"): kernels of other streams that still read the old map must have finished, as for a re-insert
  if (m->buckets.ptr) GP_HIP(hipDeviceSynchronize());
  for (int id = 0; id < gp_voxelmap::kGblocks; id++) m->arrays[id].dev.swap(fresh[id].dev);
  m->gblocks.swap(blocks);
  m->grid = g;
  m->has_grid = V > 0;
  if (!m->has_grid) m->gblocks.release();
  m->info.num_voxels = V;
  m->info.num_buckets = (int)num_buckets;
  m->has_sums = true;
  m->lru_counter = counter;
  m->generation++;
  m->plines.release();
  m->private_built = false;  // (built when a batch first asks for it: gp_voxelmap::ensure_private_table)
  if (!m->has_grid) {        // an empty map has no grid to look voxels up in: the line table, as after an empty one-shot insert
    GP_TRY(gp::build_private_table(m, s));
    GP_HIP(hipStreamSynchronize(s));
  }
  return GP_OK;
}

int gp_voxelmap_set_lru(gp_voxelmap_t* map, int64_t horizon, int64_t clear_cycle) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_set_lru: null map");
  if (horizon < 0 || clear_cycle < 1) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_set_lru: lru_horizon must be >= 0 and lru_clear_cycle >= 1");
  map->lru_horizon = horizon;
  map->lru_clear_cycle = clear_cycle;
  return GP_OK;
}

int gp_voxelmap_lru_get(const gp_voxelmap_t* map, int64_t* counter, int64_t* horizon, int64_t* clear_cycle) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_lru_get: null map");
  if (counter) *counter = map->lru_counter;
  if (horizon) *horizon = map->lru_horizon;
  if (clear_cycle) *clear_cycle = map->lru_clear_cycle;
  return GP_OK;
}

int gp_voxelmap_download_stamps(const gp_voxelmap_t* map, int64_t* out_host) {
  if (!map) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_download_stamps: null map");
  if (!map->loaded()) return gp::fail(GP_ERROR_NOT_LOADED, "gp_voxelmap_download_stamps: voxel map is not on the GPU");
  if (map->info.num_voxels > 0 && !map->has_sums) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_download_stamps: the map took no incremental insert and has no stamps");
  const size_t bytes = map->array_bytes(gp_voxelmap::kStamps);
  if (bytes == 0) return GP_OK;
  if (!out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelmap_download_stamps: null output");
  GP_HIP(hipMemcpyAsync(out_host, map->voxel_stamps.ptr, bytes, hipMemcpyDeviceToHost, map->stream));
  GP_HIP(hipStreamSynchronize(map->stream));
  return GP_OK;
}

}  // extern "C"
