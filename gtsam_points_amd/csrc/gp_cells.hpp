// gp_cells.hpp -- which cell a point belongs to, and the bounding box of a set of cells: written once for every structure that sorts points into cells.
//
// The cell rules of the library.  The first is THE rule and lives here; the other three are different rules by the reference and stay with their one user:
//   rule          cell of coordinate p                               no cell when                   used by                                          why it differs
//   cell_of       fast_floor(double(p) * inv)                        !(|p * inv| < 1e9), NaN, inf   bin_points (k-NN grids, covariances, normals),   the CPU voxel map's rule (gaussian_voxelmap_cpu.cpp:59-61);
//                                                                                                   both voxel-map builds, the incremental insert;   the voxel map and the binning must agree to the bit
//                                                                                                   hashed_cell (its range test; then clamped)
//   sample_coord  fast_floor(double(p) * inv)                        outside [-2^20, 2^20)          gp_sampling.hip                                  the reference's 21-bit voxel-grid key (point_cloud_cpu_funcs.cpp:132-146)
//   fpfh_cell     floor(double(p) / radius), clamped to +-(2^20-3)   a non-finite coordinate        gp_fpfh.hip                                      a division, as the f64 restatement of the radius search states it
//   occ_cell      fast_floor((pose * p) * inv) + 2^20, 21-bit mask   a non-finite pose * p          gp_occupancy.hpp                                 FastOccupancyGrid: pose first, no FMA, coordinates alias by the mask
//
// CellBox is the integer bounding box of cells (or blocks): the neutral box, add, merge, and on the device the reduce over the wave, the fold over the four waves of
// a workgroup and the 32-byte record a workgroup leaves in a host-mapped slot; the host's half of that hand-over is collect_boxes (gp_host.hpp, beside HostSlots).
// Outside __HIPCC__ it needs no HIP header: a host compiler builds it alone (tests/key_table_cases.cpp).
#pragma once

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GP_CELLS_HD __host__ __device__ __forceinline__
#else
#define GP_CELLS_HD inline
#endif

#include <cmath>

namespace gp {

// fast_floor in DOUBLE, util/fast_floor.hpp:12-15 (the CPU map's rule; the reference GPU map floors float(x)/float(res): ~5e-5 of points cross a voxel face)
GP_CELLS_HD int fast_floor(double x) {
  const int n = (int)x;
  return n - (x < (double)n);
}

// finite and inside the range a 32-bit cell coordinate can hold (with room for the >> 2 block arithmetic); false for NaN / inf
constexpr double kCellLimit = 1.0e9;
GP_CELLS_HD bool cell_in_range(double u) { return fabs(u) < kCellLimit; }
GP_CELLS_HD bool cell_in_range(double ux, double uy, double uz) { return cell_in_range(ux) && cell_in_range(uy) && cell_in_range(uz); }

// THE cell rule: a point has a cell iff all three |p * inv| < 1e9 ((int)NaN is 0 on the device, an infinity saturates: a caller must honour the return value)
GP_CELLS_HD bool cell_of(double px, double py, double pz, double inv, int& cx, int& cy, int& cz) {
  const double ux = px * inv, uy = py * inv, uz = pz * inv;
  const bool ok = cell_in_range(ux, uy, uz);
  cx = ok ? fast_floor(ux) : 0;
  cy = ok ? fast_floor(uy) : 0;
  cz = ok ? fast_floor(uz) : 0;
  return ok;
}

struct CellBox {
  int lo[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff}, hi[3] = {(int)0x80000000, (int)0x80000000, (int)0x80000000};  // the neutral box: merging it changes nothing

  GP_CELLS_HD bool empty() const { return lo[0] > hi[0]; }
  GP_CELLS_HD void add(const int c[3]) {
    for (int a = 0; a < 3; a++) {
      lo[a] = c[a] < lo[a] ? c[a] : lo[a];
      hi[a] = c[a] > hi[a] ? c[a] : hi[a];
    }
  }
  // row = {lo xyz, hi xyz}: the layout of every box the library stores
  GP_CELLS_HD void merge(const int row[6]) {
    for (int a = 0; a < 3; a++) {
      lo[a] = row[a] < lo[a] ? row[a] : lo[a];
      hi[a] = row[3 + a] > hi[a] ? row[3 + a] : hi[a];
    }
  }
  template <typename Int>  // (int, or the volatile int of a host-mapped slot)
  GP_CELLS_HD void store(Int* row) const {
    for (int a = 0; a < 3; a++) row[a] = lo[a], row[3 + a] = hi[a];
  }

#if defined(__HIPCC__)
  // the box of the whole wave, in every lane
  __device__ __forceinline__ void wave_reduce() {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1)
#pragma unroll
      for (int a = 0; a < 3; a++) {
        lo[a] = min(lo[a], __shfl_xor(lo[a], off, 64));
        hi[a] = max(hi[a], __shfl_xor(hi[a], off, 64));
      }
  }
  // the box of a workgroup of four waves, valid in thread 0 (wave_box: LDS; one barrier)
  __device__ __forceinline__ void block_reduce(int (*wave_box)[6]) {
    wave_reduce();
    if ((threadIdx.x & 63) == 0) store(wave_box[threadIdx.x >> 6]);
    __syncthreads();
    if (threadIdx.x == 0) {
#pragma unroll
      for (int w = 1; w < 4; w++) merge(wave_box[w]);  // (wave 0's is this thread's own)
    }
  }
  // thread 0's half of the hand-over to the host: the workgroup's 32-byte record {lo xyz, hi x | hi y, hi z, extra, seq} in its slot of host-mapped memory
  __device__ __forceinline__ void publish(int* slots /* host-mapped */, int extra, int seq) const {
    int4* slot = reinterpret_cast<int4*>(slots + 8 * (size_t)blockIdx.x);
    slot[0] = make_int4(lo[0], lo[1], lo[2], hi[0]);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // the first half is in host memory before the half that carries the sequence number
    slot[1] = make_int4(hi[1], hi[2], extra, seq);
  }
#endif
};

}  // namespace gp
#undef GP_CELLS_HD
