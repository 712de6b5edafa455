// gp_voxelmap_kernels.hpp -- the kernels of the voxel-map build, included by the two units that launch them: gp_voxelmap.hip (the one-shot builds) and
// gp_voxelmap_incremental.hip (the incremental insert, which shares the grid and bucket kernels).  Every kernel is `inline`, so that both units may hold it:
//   * shared by both builds: voxel_of / point_coord (which voxel a point belongs to) and intensity_max
//   * the hashed build, reference-shaped -- the FALLBACK for a cloud whose box exceeds the block grid, for an empty cloud and for A/B (GP_TUNE_MAP_BUILD):
//     claim_buckets_kernel, assign_voxels_kernel, accumulate_kernel (native f64 atomics relative to the voxel centre: not bit-reproducible), finalize_kernel
//   * the line table of the hashed VGICP kernel family: line_claim_kernel
//   * the occupancy-block grid of a hashed build: coords_bbox_kernel, grid_mark_kernel, grid_count_kernel, grid_renumber_kernel, buckets_renumber_kernel
//   * the binned build, the DEFAULT: segmented_stats_kernel (an ordered segmented sum, no atomics: bit-identical from run to run) and insert_voxels_kernel
//   * the incremental insert: segmented_sums_kernel (the same sum, not finalized), survivors_bbox_kernel, grid_mark_survivors_kernel, merge_source_kernel,
//     merge_finalize_kernel
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

// A point belongs to a voxel iff all three |p / leaf| < 1e9: the binned build's rule (gp_binning.hip, point_cell), false for NaN / inf.  Both builds apply it:
// on the device (int)NaN is 0, i.e. voxel (0, 0, 0), and an infinite coordinate saturates into a voxel of its own.
__device__ __forceinline__ bool voxel_of(double px, double py, double pz, double inv_leaf, int& cx, int& cy, int& cz) {
  const double ux = px * inv_leaf, uy = py * inv_leaf, uz = pz * inv_leaf;
  const bool ok = fabs(ux) < 1.0e9 && fabs(uy) < 1.0e9 && fabs(uz) < 1.0e9;
  cx = ok ? fast_floor(ux) : 0;
  cy = ok ? fast_floor(uy) : 0;
  cz = ok ? fast_floor(uz) : 0;
  return ok;
}
__device__ __forceinline__ bool point_coord(const float* __restrict__ points, int i, double inv_leaf, int& cx, int& cy, int& cz) {
  return voxel_of((double)points[3 * (size_t)i], (double)points[3 * (size_t)i + 1], (double)points[3 * (size_t)i + 2], inv_leaf, cx, cy, cz);
}

// Voxel intensity, ONE rule for both builds: the CPU map's std::max from 0.0 (gaussian_voxelmap_cpu.cpp:34-35), `cur < x ? x : cur` -- a negative value, -0.0 and a
// NaN leave +0.0.  (The reference's GPU map takes atomicMax of the bit patterns from 0, :138-139, which is the same for x >= +0 and lets every negative value, -0.0
// and NaN win otherwise.)
__device__ __forceinline__ float intensity_max(float cur, float x) { return cur < x ? x : cur; }

// voxel_bucket_assignment_kernel (gaussian_voxelmap_gpu.cu:37-75): claim a bucket per distinct voxel coordinate.
// rep[b] = index of the first point that claimed bucket b, or -1.
inline __global__ void __launch_bounds__(256) claim_buckets_kernel(const float* __restrict__ points, int n, int* __restrict__ rep, uint32_t num_buckets,
                                                            uint32_t mask, int max_scan, double inv_leaf, int* __restrict__ invalid,
                                                            int* __restrict__ failures) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  int cx, cy, cz;
  if (!point_coord(points, i, inv_leaf, cx, cy, cz)) {  // neither a member nor a failure: counted apart, so that the drop rate is over the valid points
    atomicAdd(invalid, 1);
    return;
  }
  const uint64_t hash = coord_hash(cx, cy, cz);
  for (int j = 0; j < max_scan; j++) {
    const uint32_t b = bucket_index(hash, j, num_buckets, mask);
    const int old = atomicCAS(&rep[b], -1, i);
    if (old < 0) return;  // claimed an empty bucket
    int ox, oy, oz;
    point_coord(points, old, inv_leaf, ox, oy, oz);  // (a representative is a valid point: only those claim)
    if (ox == cx && oy == cy && oz == cz) return;  // voxel already present
  }
  atomicAdd(failures, 1);  // probe chain exhausted: this point is dropped (gaussian_voxelmap_gpu.cu:67)
}

// voxel_coord_select_kernel (:77-90) + voxel id allocation (:57-60)
inline __global__ void __launch_bounds__(256) assign_voxels_kernel(const float* __restrict__ points, const int* __restrict__ rep, uint32_t num_buckets,
                                                            double inv_leaf, gp_voxel_bucket* __restrict__ buckets, int* __restrict__ voxel_coords,
                                                            int* __restrict__ num_voxels) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= num_buckets) return;
  const int r = rep[b];
  int4 out = make_int4(0, 0, 0, -1);
  if (r >= 0) {
    int cx, cy, cz;
    point_coord(points, r, inv_leaf, cx, cy, cz);
    const int v = atomicAdd(num_voxels, 1);
    out = make_int4(cx, cy, cz, v);
    voxel_coords[3 * (size_t)v] = cx;
    voxel_coords[3 * (size_t)v + 1] = cy;
    voxel_coords[3 * (size_t)v + 2] = cz;
  }
  reinterpret_cast<int4*>(buckets)[b] = out;
}

// accumulate_points_kernel (:92-152): sums[v] = { sum(p - centre) (3), sum upper(C) (6) } in double, count, max intensity
inline __global__ void __launch_bounds__(256) accumulate_kernel(const float* __restrict__ points, const float* __restrict__ covs,
                                                         const float* __restrict__ intensities, int n, VoxelMapView map, double* __restrict__ sums,
                                                         int* __restrict__ counts, unsigned int* __restrict__ intensity_bits) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  int cx, cy, cz;
  if (!voxel_of(px, py, pz, map.inv_leaf, cx, cy, cz)) return;  // NaN / inf / out of range: in no voxel
  const int v = lookup_voxel(map, cx, cy, cz);
  if (v < 0) return;  // dropped at table build
  double ox, oy, oz;
  voxel_center(map, cx, cy, cz, ox, oy, oz);
  const float* c = covs + 9 * (size_t)i;
  double* s = sums + 9 * (size_t)v;
  unsafeAtomicAdd(s + 0, px - ox);
  unsafeAtomicAdd(s + 1, py - oy);
  unsafeAtomicAdd(s + 2, pz - oz);
  unsafeAtomicAdd(s + 3, (double)c[0]);  // xx
  unsafeAtomicAdd(s + 4, 0.5 * ((double)c[3] + (double)c[1]));  // xy: symmetric part of the column-major 3x3 (the input itself when symmetric)
  unsafeAtomicAdd(s + 5, 0.5 * ((double)c[6] + (double)c[2]));  // xz
  unsafeAtomicAdd(s + 6, (double)c[4]);                         // yy
  unsafeAtomicAdd(s + 7, 0.5 * ((double)c[7] + (double)c[5]));  // yz
  unsafeAtomicAdd(s + 8, (double)c[8]);  // zz
  atomicAdd(counts + v, 1);
  if (intensities) {
    // intensity_max over the voxel, from +0.0: only x > 0 can change it, and among positive floats (inf included) the order of the bit patterns is the order of
    // the values -- atomicMax on the bits (:138-139) of those alone
    const float x = intensities[i];
    if (x > 0.0f) atomicMax(intensity_bits + v, __float_as_uint(x));
  }
}

// finalize_voxels_kernel (:154-172): divide by the count; emit the gather record and the reference-visible arrays
inline __global__ void __launch_bounds__(256) finalize_kernel(int num_voxels, double leaf, const int* __restrict__ voxel_coords, const double* __restrict__ sums,
                                                       const int* __restrict__ counts, VoxelRecord* __restrict__ records,
                                                       float* __restrict__ voxel_means, float* __restrict__ voxel_covs) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int n = counts[v];
  const double inv_n = 1.0 / (double)n;
  const double* s = sums + 9 * (size_t)v;
  const double lx = s[0] * inv_n, ly = s[1] * inv_n, lz = s[2] * inv_n;
  VoxelRecord rec;
  rec.mean_local[0] = (float)lx;
  rec.mean_local[1] = (float)ly;
  rec.mean_local[2] = (float)lz;
  rec.num_points = n;
  for (int k = 0; k < 6; k++) rec.cov[k] = s[3 + k] / (double)n;
  records[v] = rec;
  const double ox = ((double)voxel_coords[3 * (size_t)v] + 0.5) * leaf;
  const double oy = ((double)voxel_coords[3 * (size_t)v + 1] + 0.5) * leaf;
  const double oz = ((double)voxel_coords[3 * (size_t)v + 2] + 0.5) * leaf;
  voxel_means[3 * (size_t)v] = (float)(ox + lx);
  voxel_means[3 * (size_t)v + 1] = (float)(oy + ly);
  voxel_means[3 * (size_t)v + 2] = (float)(oz + lz);
  float* c = voxel_covs + 9 * (size_t)v;
  c[0] = (float)rec.cov[0];
  c[1] = c[3] = (float)rec.cov[1];
  c[2] = c[6] = (float)rec.cov[2];
  c[4] = (float)rec.cov[3];
  c[5] = c[7] = (float)rec.cov[4];
  c[8] = (float)rec.cov[5];
}

// line table: claim the first free key slot of the home line (front to back), else walk to the next line
inline __global__ void __launch_bounds__(256) line_claim_kernel(int num_voxels, const int* __restrict__ voxel_coords, gp_voxel_bucket* __restrict__ lines, uint32_t lmask) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = voxel_coords[3 * (size_t)v], cy = voxel_coords[3 * (size_t)v + 1], cz = voxel_coords[3 * (size_t)v + 2];
  uint32_t l = coord_hash32(cx, cy, cz) & lmask;
  for (;;) {
    gp_voxel_bucket* line = lines + 4 * (size_t)l;
    for (int t = 0; t < 4; t++) {
      if (atomicCAS(&line[t].voxel_index, -1, v) == -1) {
        line[t].coord[0] = cx;
        line[t].coord[1] = cy;
        line[t].coord[2] = cz;
        return;
      }
    }
    l = (l + 1) & lmask;
  }
}

// ---- occupancy-block grid (gp_device.hpp: GridBlock; geometry helpers in gp_binning.hpp) ----

// bounding box of the voxel coordinates in block units: bbox[0..2] = min, bbox[3..5] = max (wave reduce + one atomic per wave)
inline __global__ void __launch_bounds__(256) coords_bbox_kernel(int num_voxels, const int* __restrict__ voxel_coords, int* __restrict__ bbox) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const int u = v < num_voxels ? v : num_voxels - 1;
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) lo[a] = hi[a] = voxel_coords[3 * (size_t)u + a] >> 2;
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
    }
  if ((threadIdx.x & 63) == 0) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      atomicMin(bbox + a, lo[a]);
      atomicMax(bbox + 3 + a, hi[a]);
    }
  }
}

inline __global__ void __launch_bounds__(256) grid_mark_kernel(int num_voxels, const int* __restrict__ voxel_coords, GridGeom g, GridBlock* __restrict__ blocks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = voxel_coords[3 * (size_t)v], cy = voxel_coords[3 * (size_t)v + 1], cz = voxel_coords[3 * (size_t)v + 2];
  atomicOr(&blocks[grid_block_index(g, cx, cy, cz)].bits, 1ull << grid_bit(cx, cy, cz));
}

inline __global__ void __launch_bounds__(256) grid_count_kernel(long long num_blocks, GridBlock* __restrict__ blocks) {
  const long long b = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (b < num_blocks) blocks[b].base = __popcll(blocks[b].bits);
}

// new index of every voxel = base of its block + number of occupied bits below its own; coordinates move to the new order
inline __global__ void __launch_bounds__(256) grid_renumber_kernel(int num_voxels, const int* __restrict__ coords_old, GridGeom g, const GridBlock* __restrict__ blocks,
                                                            int* __restrict__ perm, int* __restrict__ coords_new) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = coords_old[3 * (size_t)v], cy = coords_old[3 * (size_t)v + 1], cz = coords_old[3 * (size_t)v + 2];
  const GridBlock blk = blocks[grid_block_index(g, cx, cy, cz)];
  const int nv = blk.base + __popcll(blk.bits & ((1ull << grid_bit(cx, cy, cz)) - 1ull));
  perm[v] = nv;
  coords_new[3 * (size_t)nv] = cx;
  coords_new[3 * (size_t)nv + 1] = cy;
  coords_new[3 * (size_t)nv + 2] = cz;
}

inline __global__ void __launch_bounds__(256) buckets_renumber_kernel(uint32_t num_buckets, gp_voxel_bucket* __restrict__ buckets, const int* __restrict__ perm) {
  const uint32_t b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= num_buckets) return;
  const int v = buckets[b].voxel_index;
  if (v >= 0) buckets[b].voxel_index = perm[v];
}

// ---- binned build (gp_binning.hpp): per-voxel statistics as an ORDERED segmented sum ----------------------------------------
// Sixteen lanes per voxel, sixteen voxels per workgroup (rounds 2-3: one wave per voxel -- the median voxel of a scan holds three points, the mean 10-30, so three
// quarters of a wave's lanes idled through nine six-step butterflies: 114 us per 2 M points, the largest kernel of the map build).  The rows of a voxel's points are
// a random gather through the sort order (12 + 36 B from wherever the point lies in the caller's arrays); when the lanes of a voxel fetched their own rows, the wave
// waited for its longest voxel with most lanes idle (68 us per 2 M points at 2.3 TB/s of fabric traffic: latency-bound).  Now the WHOLE workgroup gathers the rows of
// its sixteen voxels -- one contiguous range of the sort order, every lane busy, two rows per lane in flight -- into LDS, 512 rows at a time, and the voxels' lanes
// sum from LDS.  Lane l of a voxel adds the voxel's points l, l + 16, ... in ascending order (stable sort: ascending point index), one fixed butterfly joins the
// sixteen lanes at the end: the statistics are bit-identical from run to run (no atomics) and do not depend on where the 512-row batches fall.
// sums relative to the voxel centre in f64, like accumulate_kernel; outputs as finalize_kernel.
constexpr int kStatsBatch = 512;
// what the sixteen lanes of a voxel hold after the sum; `writer` is true in the one lane that emits the voxel
struct SegmentSums {
  int v, n;                 // voxel (cell) ordinal, its points
  int cx, cy, cz;           // its coordinate
  double ox, oy, oz;        // its centre
  double acc[9];            // sum(p - centre), upper triangle of sum(sym(C))
  float imax;               // intensity_max from +0.0
};
// the sum itself, shared by segmented_stats_kernel (the one-shot build: finalized records) and segmented_sums_kernel (the incremental insert: the raw sums)
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
      ox = ((double)cx + 0.5) * leaf, oy = ((double)cy + 0.5) * leaf, oz = ((double)cz + 0.5) * leaf;
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

inline __global__ void __launch_bounds__(256) segmented_stats_kernel(const float* __restrict__ points, const float* __restrict__ covs, const float* __restrict__ intensities,
                                                              int num_voxels, const int* __restrict__ cell_start, const int* __restrict__ order, double inv_leaf, double leaf,
                                                              VoxelRecord* __restrict__ records, int* __restrict__ num_points, float* __restrict__ voxel_means,
                                                              float* __restrict__ voxel_covs, float* __restrict__ voxel_intensities, int* __restrict__ voxel_coords,
                                                              const gp::FillJob fill_buckets) {
  gp::run_fill_job(fill_buckets);  // (the bucket table the insertion kernel behind this one claims its slots in: 0xff = empty)
  SegmentSums sum;
  if (!segmented_sums(points, covs, intensities, num_voxels, cell_start, order, inv_leaf, leaf, sum)) return;
  const int v = sum.v, n = sum.n, cx = sum.cx, cy = sum.cy, cz = sum.cz;
  const double ox = sum.ox, oy = sum.oy, oz = sum.oz;
  const double* acc = sum.acc;
  const float imax = sum.imax;
  const double inv_n = 1.0 / (double)n;
  VoxelRecord rec;
  const double lx = acc[0] * inv_n, ly = acc[1] * inv_n, lz = acc[2] * inv_n;
  rec.mean_local[0] = (float)lx;
  rec.mean_local[1] = (float)ly;
  rec.mean_local[2] = (float)lz;
  rec.num_points = n;
  for (int k = 0; k < 6; k++) rec.cov[k] = acc[3 + k] / (double)n;
  records[v] = rec;
  num_points[v] = n;
  voxel_means[3 * (size_t)v] = (float)(ox + lx);
  voxel_means[3 * (size_t)v + 1] = (float)(oy + ly);
  voxel_means[3 * (size_t)v + 2] = (float)(oz + lz);
  float* c = voxel_covs + 9 * (size_t)v;
  c[0] = (float)rec.cov[0];
  c[1] = c[3] = (float)rec.cov[1];
  c[2] = c[6] = (float)rec.cov[2];
  c[4] = (float)rec.cov[3];
  c[5] = c[7] = (float)rec.cov[4];
  c[8] = (float)rec.cov[5];
  voxel_intensities[v] = imax;
  voxel_coords[3 * (size_t)v] = cx;
  voxel_coords[3 * (size_t)v + 1] = cy;
  voxel_coords[3 * (size_t)v + 2] = cz;
}

// reference-visible bucket table from the list of DISTINCT voxels: claim the first free bucket of the probe chain
// (reference hash + max_bucket_scan_count rule, so lookup_voxel finds it); failed[0] += points of a voxel whose chain is full
inline __global__ void __launch_bounds__(256) insert_voxels_kernel(int num_voxels, const int* __restrict__ voxel_coords, const int* __restrict__ num_points,
                                                            gp_voxel_bucket* __restrict__ buckets, uint32_t num_buckets, uint32_t mask, int max_scan,
                                                            int* __restrict__ failed) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num_voxels) return;
  const int cx = voxel_coords[3 * (size_t)v], cy = voxel_coords[3 * (size_t)v + 1], cz = voxel_coords[3 * (size_t)v + 2];
  const uint64_t hash = coord_hash(cx, cy, cz);
  for (int j = 0; j < max_scan; j++) {
    gp_voxel_bucket* b = buckets + bucket_index(hash, j, num_buckets, mask);
    if (atomicCAS(&b->voxel_index, -1, v) == -1) {
      b->coord[0] = cx;
      b->coord[1] = cy;
      b->coord[2] = cz;
      return;
    }
  }
  *failed = 1;  // (a flag, not a count: the caller doubles the table until nothing fails; host-mapped on the binned build's path)
}

// ---- incremental insert (gp_voxelmap_incremental.hip): a voxel-level merge of the map's voxels with the cells of the new frame ------------------------------
// The frame is binned like a one-shot build's cloud; segmented_sums_kernel leaves each of its cells' count, f64 sums, intensity and coordinate.  The surviving old
// voxels and the new cells mark their bits in a FRESH block grid over the union box; a voxel of the merged map is a set bit, numbered in (block, bit) order like
// every map.  merge_source_kernel writes, per merged voxel, which old voxel and which new cell it is made of (-1: none); merge_finalize_kernel gathers the two, adds
// old + new in f64 and emits everything the map keeps of a voxel.  No atomics on sums: two maps fed the same frames hold the same bits.

// the eviction rule of IncrementalVoxelMap::insert (ann/impl/incremental_voxelmap_impl.hpp:49-55) for a voxel the new frame does NOT touch: `counter` is
// lru_counter after its increment; evict = the call is a clearing one (counter % lru_clear_cycle == 0)
__device__ __forceinline__ bool voxel_survives(long long stamp, int evict, long long horizon, long long counter) { return !evict || stamp + horizon >= counter; }

__device__ __forceinline__ bool grid_contains(const GridGeom& g, int cx, int cy, int cz) {
  const int bx = (cx >> 2) - g.lo[0], by = (cy >> 2) - g.lo[1], bz = (cz >> 2) - g.lo[2];
  return bx >= 0 && bx < g.dim[0] && by >= 0 && by < g.dim[1] && bz >= 0 && bz < g.dim[2];
}

// the sums of the frame's cells, as segmented_stats_kernel forms them (same lanes, same order), not finalized
inline __global__ void __launch_bounds__(256) segmented_sums_kernel(const float* __restrict__ points, const float* __restrict__ covs, const float* __restrict__ intensities,
                                                                    int num_cells, const int* __restrict__ cell_start, const int* __restrict__ order, double inv_leaf,
                                                                    double leaf, int* __restrict__ cell_counts, double* __restrict__ cell_sums,
                                                                    float* __restrict__ cell_intensities, int* __restrict__ cell_coords) {
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

// coords_bbox_kernel over the voxels that survive a clearing call (an evicted voxel contributes the empty box)
inline __global__ void __launch_bounds__(256) survivors_bbox_kernel(int num_voxels, const int* __restrict__ voxel_coords, const long long* __restrict__ stamps,
                                                                    long long horizon, long long counter, int* __restrict__ bbox) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  const bool alive = v < num_voxels && voxel_survives(stamps[v], 1, horizon, counter);
  int lo[3], hi[3];
#pragma unroll
  for (int a = 0; a < 3; a++) {
    const int b = alive ? voxel_coords[3 * (size_t)v + a] >> 2 : 0;
    lo[a] = alive ? b : 0x7fffffff;
    hi[a] = alive ? b : (int)0x80000000;
  }
#pragma unroll
  for (int off = 32; off > 0; off >>= 1)
#pragma unroll
    for (int a = 0; a < 3; a++) {
      lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
      hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
    }
  if ((threadIdx.x & 63) == 0 && lo[0] <= hi[0]) {
#pragma unroll
    for (int a = 0; a < 3; a++) {
      atomicMin(bbox + a, lo[a]);
      atomicMax(bbox + 3 + a, hi[a]);
    }
  }
}

// grid_mark_kernel with the eviction rule: the old voxels that survive mark their bits in the new grid (stamps == null: the frame's cells, which all do).
// The new box holds every survivor and every cell by construction; a coordinate outside it marks nothing
inline __global__ void __launch_bounds__(256) grid_mark_survivors_kernel(int num, const int* __restrict__ coords, const long long* __restrict__ stamps, int evict,
                                                                         long long horizon, long long counter, GridGeom g, GridBlock* __restrict__ blocks) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num) return;
  if (stamps && !voxel_survives(stamps[v], evict, horizon, counter)) return;
  const int cx = coords[3 * (size_t)v], cy = coords[3 * (size_t)v + 1], cz = coords[3 * (size_t)v + 2];
  if (!grid_contains(g, cx, cy, cz)) return;
  atomicOr(&blocks[grid_block_index(g, cx, cy, cz)].bits, 1ull << grid_bit(cx, cy, cz));
}

// source[new index] = v for every old voxel (or new cell) v whose bit is set in the new grid.  For an old voxel that is: it survived by its stamp, or the frame
// touches it (the cell set the bit) -- exactly the voxels the reference keeps, whose stamp of a touched voxel is the current counter.  An evicted voxel may lie
// outside the new box
inline __global__ void __launch_bounds__(256) merge_source_kernel(int num, const int* __restrict__ coords, GridGeom g, const GridBlock* __restrict__ blocks,
                                                                  int* __restrict__ source) {
  const int v = blockIdx.x * blockDim.x + threadIdx.x;
  if (v >= num) return;
  const int cx = coords[3 * (size_t)v], cy = coords[3 * (size_t)v + 1], cz = coords[3 * (size_t)v + 2];
  if (!grid_contains(g, cx, cy, cz)) return;
  const GridBlock blk = blocks[grid_block_index(g, cx, cy, cz)];
  const unsigned long long bit = 1ull << grid_bit(cx, cy, cz);
  if (!(blk.bits & bit)) return;
  source[blk.base + __popcll(blk.bits & (bit - 1ull))] = v;
}

// the old map's per-voxel arrays, and the frame's per-cell arrays, as merge_finalize_kernel gathers them
struct MergeOld {
  const int* coords;
  const int* counts;
  const double* sums;
  const long long* stamps;
  const float* intensities;
};
struct MergeNew {
  const int* coords;
  const int* counts;
  const double* sums;
  const float* intensities;
};
// one thread per voxel of the merged map: old + new in f64 (a voxel of one source alone keeps that source's sums to the bit), then the division and the outputs of
// segmented_stats_kernel
inline __global__ void __launch_bounds__(256) merge_finalize_kernel(int num_voxels, const int* __restrict__ source_old, const int* __restrict__ source_new, MergeOld old,
                                                                    MergeNew cell, long long stamp_now, double leaf, double* __restrict__ sums,
                                                                    long long* __restrict__ stamps, VoxelRecord* __restrict__ records, int* __restrict__ num_points,
                                                                    float* __restrict__ voxel_means, float* __restrict__ voxel_covs,
                                                                    float* __restrict__ voxel_intensities, int* __restrict__ voxel_coords,
                                                                    const gp::FillJob fill_buckets) {
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
  const double inv_n = 1.0 / (double)n;
  VoxelRecord rec;
  const double lx = acc[0] * inv_n, ly = acc[1] * inv_n, lz = acc[2] * inv_n;
  rec.mean_local[0] = (float)lx;
  rec.mean_local[1] = (float)ly;
  rec.mean_local[2] = (float)lz;
  rec.num_points = n;
#pragma unroll
  for (int k = 0; k < 6; k++) rec.cov[k] = acc[3 + k] / (double)n;
  records[v] = rec;
  num_points[v] = n;
  const double ox = ((double)cx + 0.5) * leaf, oy = ((double)cy + 0.5) * leaf, oz = ((double)cz + 0.5) * leaf;
  voxel_means[3 * (size_t)v] = (float)(ox + lx);
  voxel_means[3 * (size_t)v + 1] = (float)(oy + ly);
  voxel_means[3 * (size_t)v + 2] = (float)(oz + lz);
  float* c = voxel_covs + 9 * (size_t)v;
  c[0] = (float)rec.cov[0];
  c[1] = c[3] = (float)rec.cov[1];
  c[2] = c[6] = (float)rec.cov[2];
  c[4] = (float)rec.cov[3];
  c[5] = c[7] = (float)rec.cov[4];
  c[8] = (float)rec.cov[5];
  voxel_intensities[v] = imax;
  voxel_coords[3 * (size_t)v] = cx;
  voxel_coords[3 * (size_t)v + 1] = cy;
  voxel_coords[3 * (size_t)v + 2] = cz;
}

}  // namespace gp
