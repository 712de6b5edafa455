// gp_voxelmap_kernels.hpp -- the device functions of the voxel-map build, shared by the kernels of the two units that build maps: gp_voxelmap.hip (the one-shot builds,
// the block grid and the bucket placement) and gp_voxelmap_incremental.hip (the incremental insert).  No kernel lives here: each is in the unit that launches it.
//   * point_coord (which voxel a point belongs to: cell_of, gp_cells.hpp) and intensity_max
//   * segmented_sums: the ordered segmented sum of the binned build (no atomics: bit-identical from run to run)
//   * emit_voxel_stats / emit_voxel: ONE rule that turns a voxel's count, f64 sums and coordinate into the gather record and the reference-visible arrays
//   * grid_contains / grid_ordinal: the block grid's bounds check and its numbering rule
//   * VoxelSet / voxel_survives: a list of voxel coordinates, optionally thinned by the LRU eviction rule
//
// Replaces the thrust::for_each functors of src/gtsam_points/types/gaussian_voxelmap_gpu.cu:25-172.  Differences by design:
//   * voxel coordinates are floor(double(p) * (1.0/leaf)) -- the CPU map's rule (gaussian_voxelmap_cpu.cpp:59-61)
//   * statistics are sums in f64 relative to the voxel centre, not unordered f32 atomics
//   * besides the reference-visible arrays (num_points / voxel_means / voxel_covs / voxel_intensities) the map
//     keeps one aligned 64-B gather record per voxel (gp::VoxelRecord) that the VGICP kernels read
//   * no intermediate coordinate array: a bucket's representative point is re-floored when compared
#pragma once

#include "gp_binning.hpp"
#include "gp_host.hpp"

namespace gp {

// A point belongs to the voxel cell_of gives it (gp_cells.hpp: the one rule both builds and the binning share, false for NaN / inf / out of range).
__device__ __forceinline__ bool point_coord(const float* __restrict__ points, int i, double inv_leaf, int& cx, int& cy, int& cz) {
  return cell_of((double)points[3 * (size_t)i], (double)points[3 * (size_t)i + 1], (double)points[3 * (size_t)i + 2], inv_leaf, cx, cy, cz);
}

// Voxel intensity, ONE rule for both builds: the CPU map's std::max from 0.0 (gaussian_voxelmap_cpu.cpp:34-35), `cur < x ? x : cur` -- a negative value, -0.0 and a
// NaN leave +0.0.  (The reference's GPU map takes atomicMax of the bit patterns from 0, :138-139, which is the same for x >= +0 and lets every negative value, -0.0
// and NaN win otherwise.)
__device__ __forceinline__ float intensity_max(float cur, float x) { return cur < x ? x : cur; }

// ---- one voxel emit ----
// the per-voxel arrays a build writes, from rows of the map's table of arrays (the map's own, or the fresh set of an incremental insert)
struct VoxelOutputs {
  VoxelRecord* records;
  int* num_points;
  float* means;
  float* covs;
  float* intensities;
  int* coords;
};
inline VoxelOutputs voxel_outputs(const gp_voxelmap::Array* rows) {
  return {rows[gp_voxelmap::kRecords].dev.as<VoxelRecord>(), rows[gp_voxelmap::kNumPoints].dev.as<int>(), rows[gp_voxelmap::kMeans].dev.as<float>(),
          rows[gp_voxelmap::kCovs].dev.as<float>(),          rows[gp_voxelmap::kIntensities].dev.as<float>(), rows[gp_voxelmap::kCoords].dev.as<int>()};
}

// the centre of a voxel: THE expression the sums are relative to
__device__ __forceinline__ double voxel_centre(int c, double leaf) { return ((double)c + 0.5) * leaf; }

// voxel v from its count, its sums relative to the centre { sum(p - centre) (3), sum upper(C) (6) } and that centre, voxel_centre of its coordinate: the gather record,
// the mean and the 3x3 covariance.  The expression order is the maps' bits (the VGICP kernels read the records; the parity tests hold them): do not reassociate.
// (The centre comes in as a value, not as (coordinate, leaf): the lanes of segmented_sums hold it already, and segmented_stats_kernel stays the code it was)
__device__ __forceinline__ void emit_voxel_stats(const VoxelOutputs& out, int v, int n, const double* acc, double ox, double oy, double oz) {
  const double inv_n = 1.0 / (double)n;
  const double lx = acc[0] * inv_n, ly = acc[1] * inv_n, lz = acc[2] * inv_n;
  VoxelRecord rec;
  rec.mean_local[0] = (float)lx;
  rec.mean_local[1] = (float)ly;
  rec.mean_local[2] = (float)lz;
  rec.num_points = n;
#pragma unroll
  for (int k = 0; k < 6; k++) rec.cov[k] = acc[3 + k] / (double)n;
  out.records[v] = rec;
  out.means[3 * (size_t)v] = (float)(ox + lx);
  out.means[3 * (size_t)v + 1] = (float)(oy + ly);
  out.means[3 * (size_t)v + 2] = (float)(oz + lz);
  float* c = out.covs + 9 * (size_t)v;
  c[0] = (float)rec.cov[0];
  c[1] = c[3] = (float)rec.cov[1];
  c[2] = c[6] = (float)rec.cov[2];
  c[4] = (float)rec.cov[3];
  c[5] = c[7] = (float)rec.cov[4];
  c[8] = (float)rec.cov[5];
}
// ... and what the hashed build has in place before its finalize: the count, the intensity and the coordinate
__device__ __forceinline__ void emit_voxel(const VoxelOutputs& out, int v, int n, const double* acc, float imax, int cx, int cy, int cz, double ox, double oy, double oz) {
  emit_voxel_stats(out, v, n, acc, ox, oy, oz);
  out.num_points[v] = n;
  out.intensities[v] = imax;
  out.coords[3 * (size_t)v] = cx;
  out.coords[3 * (size_t)v + 1] = cy;
  out.coords[3 * (size_t)v + 2] = cz;
}

// ---- occupancy-block grid (gp_device.hpp: GridBlock; geometry helpers in gp_binning.hpp) ----

__device__ __forceinline__ bool grid_contains(const GridGeom& g, int cx, int cy, int cz) {
  const int bx = (cx >> 2) - g.lo[0], by = (cy >> 2) - g.lo[1], bz = (cz >> 2) - g.lo[2];
  return bx >= 0 && bx < g.dim[0] && by >= 0 && by < g.dim[1] && bz >= 0 && bz < g.dim[2];
}

// the numbering of every map: ordinal of a voxel = base of its block + number of occupied bits below its own; -1 when its bit is not set.  (cx, cy, cz) lies in g
__device__ __forceinline__ int grid_ordinal(const GridGeom& g, const GridBlock* __restrict__ blocks, int cx, int cy, int cz) {
  const GridBlock blk = blocks[grid_block_index(g, cx, cy, cz)];
  const unsigned long long bit = 1ull << grid_bit(cx, cy, cz);
  return (blk.bits & bit) ? blk.base + __popcll(blk.bits & (bit - 1ull)) : -1;
}

// the eviction rule of IncrementalVoxelMap::insert (ann/impl/incremental_voxelmap_impl.hpp:49-55) for a voxel the new frame does NOT touch: `counter` is
// lru_counter after its increment; evict = the call is a clearing one (counter % lru_clear_cycle == 0)
__device__ __forceinline__ bool voxel_survives(long long stamp, int evict, long long horizon, long long counter) { return !evict || stamp + horizon >= counter; }

// a list of voxel coordinates as the bounding-box and the mark kernel walk it; stamps == null: every voxel is alive (a one-shot build's voxels, a frame's cells)
struct VoxelSet {
  int num;
  const int* coords;
  const long long* stamps;
  int evict;
  long long horizon, counter;
  __device__ __forceinline__ bool alive(int v) const { return v < num && (!stamps || voxel_survives(stamps[v], evict, horizon, counter)); }
};

// ---- binned build (gp_binning.hpp): per-voxel statistics as an ORDERED segmented sum ----------------------------------------
// Sixteen lanes per voxel, sixteen voxels per workgroup (rounds 2-3: one wave per voxel -- the median voxel of a scan holds three points, the mean 10-30, so three
// quarters of a wave's lanes idled through nine six-step butterflies: 114 us per 2 M points, the largest kernel of the map build).  The rows of a voxel's points are
// a random gather through the sort order (12 + 36 B from wherever the point lies in the caller's arrays); when the lanes of a voxel fetched their own rows, the wave
// waited for its longest voxel with most lanes idle (68 us per 2 M points at 2.3 TB/s of fabric traffic: latency-bound).  Now the WHOLE workgroup gathers the rows of
// its sixteen voxels -- one contiguous range of the sort order, every lane busy, two rows per lane in flight -- into LDS, 512 rows at a time, and the voxels' lanes
// sum from LDS.  Lane l of a voxel adds the voxel's points l, l + 16, ... in ascending order (stable sort: ascending point index), one fixed butterfly joins the
// sixteen lanes at the end: the statistics are bit-identical from run to run (no atomics) and do not depend on where the 512-row batches fall.
// sums relative to the voxel centre in f64, like accumulate_kernel (gp_voxelmap.hip).
constexpr int kStatsBatch = 512;
// what the sixteen lanes of a voxel hold after the sum; segmented_sums returns true in the one lane that emits the voxel
struct SegmentSums {
  int v, n;                 // voxel (cell) ordinal, its points
  int cx, cy, cz;           // its coordinate
  double ox, oy, oz;        // its centre
  double acc[9];            // sum(p - centre), upper triangle of sum(sym(C))
  float imax;               // intensity_max from +0.0
};
// the sum itself, shared by segmented_stats_kernel (gp_voxelmap.hip, the one-shot build: finalized records) and segmented_sums_kernel (gp_voxelmap_incremental.hip: the raw sums)
__device__ __forceinline__ bool segmented_sums(const float* __restrict__ points, const float* __restrict__ covs, const float* __restrict__ intensities, int num_voxels,
                                               const int* __restrict__ cell_start, const int* __restrict__ order, double inv_leaf, double leaf, SegmentSums& out) {
  constexpr int kGroup = 16;
  __shared__ float rows[kStatsBatch][12];  // x y z, then the covariance's nine entries
  __shared__ float inten[kStatsBatch];
  const int lane = threadIdx.x & (kGroup - 1);
  const int v0 = blockIdx.x * (256 / kGroup);
  const int v1 = min(v0 + 256 / kGroup, num_voxels);
  const int v = v0 + (threadIdx.x / kGroup);
  const bool live = v < num_voxels;
  const int p0 = cell_start[v0], p1 = cell_start[v1];
  const int b = live ? cell_start[v] : p1, e = live ? cell_start[v + 1] : p1;
  int cx = 0, cy = 0, cz = 0;
  double ox = 0.0, oy = 0.0, oz = 0.0;  // the voxel's centre, from its first point -- taken from the batch that holds it (two dependent loads less in front of the gather)
  double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  float imax = 0.0f;  // intensity_max from +0.0; 0 when the cloud has no intensities
  for (int batch = p0; batch < p1; batch += kStatsBatch) {
    const int cnt = min(kStatsBatch, p1 - batch);
    float row[kStatsBatch / 256][12];
    float rit[kStatsBatch / 256];
#pragma unroll
    for (int q = 0; q < kStatsBatch / 256; q++) {
      const int r = q * 256 + (int)threadIdx.x;
      rit[q] = 0.0f;
      if (r < cnt) {
        const size_t i = (size_t)order[batch + r];
#pragma unroll
        for (int k = 0; k < 3; k++) row[q][k] = points[3 * i + k];
#pragma unroll
        for (int k = 0; k < 9; k++) row[q][3 + k] = covs[9 * i + k];
        if (intensities) rit[q] = intensities[i];
      }
    }
#pragma unroll
    for (int q = 0; q < kStatsBatch / 256; q++) {
      const int r = q * 256 + (int)threadIdx.x;
      if (r < cnt) {
#pragma unroll
        for (int k = 0; k < 12; k++) rows[r][k] = row[q][k];
        inten[r] = rit[q];
      }
    }
    __syncthreads();
    const int lo = max(b, batch), hi = min(e, batch + cnt);
    if (live && b >= batch && b < batch + cnt) {
      const float* f = rows[b - batch];
      cx = fast_floor((double)f[0] * inv_leaf), cy = fast_floor((double)f[1] * inv_leaf), cz = fast_floor((double)f[2] * inv_leaf);
      ox = voxel_centre(cx, leaf), oy = voxel_centre(cy, leaf), oz = voxel_centre(cz, leaf);
    }
    for (int j = lo + ((lane - (lo - b)) & (kGroup - 1)); j < hi; j += kGroup) {
      const float* c = rows[j - batch];
      acc[0] += (double)c[0] - ox;
      acc[1] += (double)c[1] - oy;
      acc[2] += (double)c[2] - oz;
      acc[3] += (double)c[3];
      acc[4] += 0.5 * ((double)c[6] + (double)c[4]);  // symmetric part of the column-major 3x3 (the input itself when symmetric)
      acc[5] += 0.5 * ((double)c[9] + (double)c[5]);
      acc[6] += (double)c[7];
      acc[7] += 0.5 * ((double)c[10] + (double)c[8]);
      acc[8] += (double)c[11];
      imax = intensity_max(imax, inten[j - batch]);
    }
    __syncthreads();
  }
#pragma unroll
  for (int k = 0; k < 9; k++) {
#pragma unroll
    for (int off = kGroup / 2; off > 0; off >>= 1) acc[k] += __shfl_xor(acc[k], off, kGroup);
  }
#pragma unroll
  for (int off = kGroup / 2; off > 0; off >>= 1) imax = intensity_max(imax, __shfl_xor(imax, off, kGroup));
  out.v = v;
  out.n = e - b;
  out.cx = cx, out.cy = cy, out.cz = cz;
  out.ox = ox, out.oy = oy, out.oz = oz;
#pragma unroll
  for (int k = 0; k < 9; k++) out.acc[k] = acc[k];
  out.imax = imax;
  return live && lane == 0;
}

}  // namespace gp
