// gp_occupancy.hpp -- the device side of the occupancy set (gp_occupancy.hip; host side: gp_occupancy_grid.hpp): device counterpart of FastOccupancyGrid (ann/fast_occupancy_grid.hpp:13-113,
// ann/impl/fast_occupancy_grid_impl.hpp:14-74, src/gtsam_points/ann/fast_occupancy_grid.cpp:12-93).
//
// Semantics are the reference's:
//   cell    fast_floor((pose * p) * inv_resolution) + 2^20 per axis (impl:18), in f64 on the f32 point, evaluated as ((r0 x + r1 y) + r2 z) + t without fused
//           multiply-adds (Eigen's 4x4 * (x, y, z, 1) in coefficient order), so that a host restatement in plain f64 reproduces every cell to the bit
//   block   8 x 8 x 8 cells (FastOccupancyBlock::stride), one 512-bit word group: block = cell >> 3, bit = x + 8 y + 64 z of cell & 7 (hpp:22)
//   key     the three block coordinates masked to 21 bits and packed into a uint64 (cpp:23-27).  Coordinates outside 21 bits alias by the mask, as in the reference
//           (a cell more than 2^20 cells below the origin makes the reference's truncating division and this shift disagree as well: both are outside the grid's range)
// A point with a non-finite transformed coordinate has no cell: it is not inserted and overlaps nothing (the reference floors it into an undefined integer).
//
// The table is this library's own: open addressing with linear probing over `mask + 1` slots (a power of two, at most half full: sized from the point count), slot =
// occ_hash(key) & mask, keys[slot] = kEmptyKey for a free slot, words[slot][16] the block's 512 bits.  The reference's 10-probe limit and rehash are its
// implementation, not its semantics: as a set of cells this table is exact.  The probe loops are gp_key_table.hpp's: at most mask + 1 steps, so a damaged table
// (no free slot, a key stored twice) gives a wrong count, never a spin.
#pragma once

#include "gp_device.hpp"
#include "gp_key_table.hpp"

namespace gp {

constexpr int kOccCoordOffset = 1 << 20;
constexpr unsigned long long kOccCoordMask = (1ull << 21) - 1;

struct OccupancyView {
  const unsigned long long* keys;  // [mask + 1]
  const uint32_t* words;           // [mask + 1][16]
  uint32_t mask;
  uint32_t pad_;
  double inv_resolution;
};

__host__ __device__ __forceinline__ uint32_t occ_hash(unsigned long long key) {
  unsigned long long h = key * 0x9E3779B97F4A7C15ull;
  h ^= h >> 32;
  return (uint32_t)h;
}

// (key, bit) of the cell of pose * (x, y, z); false for a point without a cell
__device__ __forceinline__ bool occ_cell(const Pose& T, double inv_resolution, float fx, float fy, float fz, unsigned long long& key, int& bit) {
#pragma clang fp contract(off)
  const double x = (double)fx, y = (double)fy, z = (double)fz;
  const double qx = ((T.r00 * x + T.r01 * y) + T.r02 * z) + T.tx;
  const double qy = ((T.r10 * x + T.r11 * y) + T.r12 * z) + T.ty;
  const double qz = ((T.r20 * x + T.r21 * y) + T.r22 * z) + T.tz;
  if (!finite3(qx, qy, qz)) return false;
  const int gx = fast_floor(qx * inv_resolution) + kOccCoordOffset;
  const int gy = fast_floor(qy * inv_resolution) + kOccCoordOffset;
  const int gz = fast_floor(qz * inv_resolution) + kOccCoordOffset;
  key = ((unsigned long long)(gx >> 3) & kOccCoordMask) | (((unsigned long long)(gy >> 3) & kOccCoordMask) << 21) | (((unsigned long long)(gz >> 3) & kOccCoordMask) << 42);
  bit = (gx & 7) | ((gy & 7) << 3) | ((gz & 7) << 6);
  return true;
}

// 1 when the cell is in the set
__device__ __forceinline__ int occ_lookup(const OccupancyView& g, unsigned long long key, int bit) {
  const int slot = key_find(g.keys, g.mask, occ_hash(key) & g.mask, key);
  return slot < 0 ? 0 : (g.words[(size_t)slot * 16 + (bit >> 5)] >> (bit & 31)) & 1u;
}

}  // namespace gp
