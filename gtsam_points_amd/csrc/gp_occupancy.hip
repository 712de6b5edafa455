// gp_occupancy.hip -- the occupancy set (FastOccupancyGrid) on the device: insertion, growth, overlap of one cloud at one pose and at a batch of poses (RANSAC's
// scoring launch).  Device counterpart of ann/fast_occupancy_grid.hpp; cell, key and lookup are gp_occupancy.hpp's, the grid and what gp_registration.hip calls are
// gp_occupancy_grid.hpp's; the contract of every entry point is in include/gtsam_points_hip.h.  The cells a host restatement has to reproduce to the bit are computed
// without fused multiply-adds: contraction is off for the whole unit.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include "gp_alignment.hpp"
#include "gp_occupancy_grid.hpp"

namespace gp {

struct Pose16 {
  double m[16];
};
static Pose16 pose_or_identity(const double* pose) {
  Pose16 p;
  set_identity16(p.m);
  if (pose) std::memcpy(p.m, pose, sizeof(p.m));
  return p;
}

// the slot of `key`, claimed if it is new (*claimed = 1); mask + 1 when the table has no room (cannot happen at half load; the caller drops the point)
__device__ __forceinline__ uint32_t occ_find_or_claim(unsigned long long* keys, uint32_t mask, unsigned long long key, int* claimed) {
  return key_claim(keys, mask, occ_hash(key) & mask, key, claimed);
}

__global__ __launch_bounds__(256) void occupancy_insert_kernel(unsigned long long* keys, uint32_t* words, uint32_t mask, double inv_resolution, const float* __restrict__ points,
                                                               int n, Pose16 pose, int* counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Pose T = load_pose(pose.m);
  int new_block = 0, new_cell = 0;
  if (i < n) {
    unsigned long long key;
    int bit;
    if (occ_cell(T, inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) {
      const uint32_t slot = occ_find_or_claim(keys, mask, key, &new_block);
      if (slot <= mask) {
        const uint32_t m = 1u << (bit & 31);
        new_cell = (atomicOr(&words[(size_t)slot * 16 + (bit >> 5)], m) & m) == 0;
      }
    }
  }
  const int blocks = wave_sum(new_block), cells = wave_sum(new_cell);
  if ((threadIdx.x & 63) == 0) {
    if (blocks) atomicAdd(&counters[0], blocks);
    if (cells) atomicAdd(&counters[1], cells);
  }
}

// moves every block of a table into a larger one (each key is stored once, so a new slot has one writer)
__global__ __launch_bounds__(256) void occupancy_rehash_kernel(const unsigned long long* __restrict__ old_keys, const uint32_t* __restrict__ old_words, uint32_t old_slots,
                                                               unsigned long long* keys, uint32_t* words, uint32_t mask) {
  const uint32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= old_slots) return;
  const unsigned long long key = old_keys[i];
  if (key == kEmptyKey) return;
  int claimed;
  const uint32_t slot = occ_find_or_claim(keys, mask, key, &claimed);
  if (slot > mask) return;
  for (int w = 0; w < 16; w++) atomicOr(&words[(size_t)slot * 16 + w], old_words[(size_t)i * 16 + w]);
}

__global__ __launch_bounds__(256) void occupancy_overlaps_kernel(OccupancyView g, const float* __restrict__ points, int n, Pose16 pose, unsigned char* overlaps, int* count) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  const Pose T = load_pose(pose.m);
  int hit = 0;
  if (i < n) {
    unsigned long long key;
    int bit;
    if (occ_cell(T, g.inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) hit = occ_lookup(g, key, bit);
    if (overlaps) overlaps[i] = (unsigned char)hit;
  }
  if (count) {
    const int hits = wave_sum(hit);
    if ((threadIdx.x & 63) == 0 && hits) atomicAdd(count, hits);
  }
}

// The scoring kernel: one workgroup = kScorePoints consecutive points of ONE hypothesis; workgroup b serves list slot b / tiles, tile b % tiles.  The pose is a
// uniform (scalar) load, the cloud (12 B per point) and the table are re-read by every hypothesis from L2 / the infinity cache; the counts are integer atomics,
// one per wave.  list == NULL: hypothesis = slot.  stop: a device flag read first (RANSAC's early stop); num_list: the number of list entries, on the device.
constexpr int kScorePoints = 1024;
__global__ __launch_bounds__(256) void occupancy_overlap_batch_kernel(OccupancyView g, const float* __restrict__ points, int n, const double* __restrict__ poses,
                                                                      const int* __restrict__ list, const int* __restrict__ num_list, int tiles, const int* __restrict__ stop,
                                                                      int* __restrict__ counts) {
  if (stop && *stop) return;
  const int slot = blockIdx.x / tiles, tile = blockIdx.x - slot * tiles;
  if (num_list && slot >= *num_list) return;
  const int h = list ? list[slot] : slot;
  const Pose T = load_pose(poses + 16 * (size_t)h);
  int hits = 0;
#pragma unroll
  for (int k = 0; k < kScorePoints / 256; k++) {
    const int i = tile * kScorePoints + k * 256 + threadIdx.x;
    if (i < n) {
      unsigned long long key;
      int bit;
      if (occ_cell(T, g.inv_resolution, points[3 * (size_t)i], points[3 * (size_t)i + 1], points[3 * (size_t)i + 2], key, bit)) hits += occ_lookup(g, key, bit);
    }
  }
  hits = wave_sum(hits);
  if ((threadIdx.x & 63) == 0 && hits) atomicAdd(&counts[h], hits);
}

int launch_overlap_batch(const gp_occupancy_grid* grid, const float* points, int n, const double* poses_dev, const int* list, const int* num_list, int num_slots, const int* stop,
                         int* counts, hipStream_t stream) {
  const int tiles = (n + kScorePoints - 1) / kScorePoints;
  if ((long long)tiles * num_slots > 0x7fffffffLL) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap_batch: num_poses x ceil(num_points / 1024) exceeds 2^31 - 1");
  hipLaunchKernelGGL(occupancy_overlap_batch_kernel, dim3((unsigned)(tiles * num_slots)), dim3(256), 0, stream, grid->view(), points, n, poses_dev, list, num_list, tiles, stop,
                     counts);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

static int grid_reserve(gp_occupancy_grid* g, int extra_points) {
  const unsigned long long need = 2ull * ((unsigned long long)g->num_blocks + (unsigned long long)extra_points);
  unsigned long long slots = 64;
  while (slots < need) slots <<= 1;
  if (slots <= g->slots) return GP_OK;
  if (slots > (1ull << 30)) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_insert: the table would exceed 2^30 slots");
  DeviceArray keys, words;
  GP_TRY(keys.alloc_pooled(slots * 8, g->stream));
  GP_TRY(words.alloc_pooled(slots * 64, g->stream));
  GP_HIP(hipMemsetAsync(keys.ptr, 0xff, slots * 8, g->stream));
  GP_HIP(hipMemsetAsync(words.ptr, 0, slots * 64, g->stream));
  if (g->slots && g->num_blocks) {
    hipLaunchKernelGGL(occupancy_rehash_kernel, dim3(blocks_of(g->slots)), dim3(256), 0, g->stream, g->keys.as<unsigned long long>(), g->words.as<uint32_t>(), g->slots,
                       keys.as<unsigned long long>(), words.as<uint32_t>(), (uint32_t)(slots - 1));
    GP_HIP(hipGetLastError());
  }
  if (g->slots) GP_HIP(hipStreamSynchronize(g->stream));  // the old table is freed below
  g->keys.swap(keys);
  g->words.swap(words);
  g->slots = (uint32_t)slots;
  return GP_OK;
}

int grid_insert(gp_occupancy_grid* g, const float* points, int n, const double* pose, bool wait) {
  if (n == 0) return GP_OK;
  GP_TRY(grid_reserve(g, n));
  hipLaunchKernelGGL(occupancy_insert_kernel, dim3(blocks_of(n)), dim3(256), 0, g->stream, g->keys.as<unsigned long long>(), g->words.as<uint32_t>(), g->slots - 1,
                     1.0 / g->resolution, points, n, pose_or_identity(pose), g->counters.as<int>());
  GP_HIP(hipGetLastError());
  if (!wait) return GP_OK;
  int c[2] = {0, 0};
  GP_HIP(hipMemcpyAsync(c, g->counters.ptr, sizeof(c), hipMemcpyDeviceToHost, g->stream));
  GP_HIP(hipStreamSynchronize(g->stream));
  g->num_blocks = c[0];
  g->num_cells = c[1];
  return GP_OK;
}

int grid_init(gp_occupancy_grid* g, double resolution, hipStream_t stream, int reserve_points) {
  g->resolution = resolution;
  g->stream = stream;
  GP_TRY(g->counters.alloc_pooled(16, stream));
  GP_HIP(hipMemsetAsync(g->counters.ptr, 0, 16, stream));
  return grid_reserve(g, reserve_points);
}

}  // namespace gp

extern "C" {

int gp_occupancy_grid_create(double resolution, gp_stream_t stream, gp_occupancy_grid_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_create: out is NULL");
  *out = nullptr;
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_create: the resolution must be positive and finite");
  auto* g = new gp_occupancy_grid();
  const int rc = gp::grid_init(g, resolution, (hipStream_t)stream);
  if (rc != GP_OK) {
    delete g;
    return rc;
  }
  *out = g;
  return GP_OK;
}

int gp_occupancy_grid_destroy(gp_occupancy_grid_t* grid) {
  delete grid;  // (waits for the grid's stream)
  return GP_OK;
}

int gp_occupancy_grid_insert(gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose) {
  if (!grid || num_points < 0 || (num_points > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_insert: bad arguments");
  return gp::grid_insert(grid, points_dev, num_points, pose);
}

int gp_occupancy_grid_overlap(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose, int* num_overlap) {
  if (!grid || !num_overlap || num_points < 0 || (num_points > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap: bad arguments");
  *num_overlap = 0;
  if (num_points == 0) return GP_OK;
  gp::DeviceArray count;
  GP_TRY(count.alloc_async(16, grid->stream));
  GP_HIP(hipMemsetAsync(count.ptr, 0, 16, grid->stream));
  hipLaunchKernelGGL(gp::occupancy_overlaps_kernel, dim3(gp::blocks_of(num_points)), dim3(256), 0, grid->stream, grid->view(), points_dev, num_points, gp::pose_or_identity(pose),
                     (unsigned char*)nullptr, count.as<int>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(num_overlap, count.ptr, sizeof(int), hipMemcpyDeviceToHost, grid->stream));
  GP_HIP(hipStreamSynchronize(grid->stream));
  return GP_OK;
}

int gp_occupancy_grid_get_overlaps(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* pose, unsigned char* overlaps_out_dev) {
  if (!grid || num_points < 0 || (num_points > 0 && (!points_dev || !overlaps_out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_get_overlaps: bad arguments");
  if (num_points == 0) return GP_OK;
  hipLaunchKernelGGL(gp::occupancy_overlaps_kernel, dim3(gp::blocks_of(num_points)), dim3(256), 0, grid->stream, grid->view(), points_dev, num_points, gp::pose_or_identity(pose),
                     overlaps_out_dev, (int*)nullptr);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_occupancy_grid_overlap_batch(const gp_occupancy_grid_t* grid, const float* points_dev, int num_points, const double* poses_dev, int num_poses, int* counts_out_dev) {
  if (!grid || num_points < 0 || num_poses < 0 || (num_points > 0 && !points_dev) || (num_poses > 0 && (!poses_dev || !counts_out_dev)))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_overlap_batch: bad arguments");
  if (num_poses == 0) return GP_OK;
  GP_HIP(hipMemsetAsync(counts_out_dev, 0, sizeof(int) * (size_t)num_poses, grid->stream));
  if (num_points == 0) return GP_OK;
  return gp::launch_overlap_batch(grid, points_dev, num_points, poses_dev, nullptr, nullptr, num_poses, nullptr, counts_out_dev, grid->stream);
}

int gp_occupancy_grid_num_occupied_cells(const gp_occupancy_grid_t* grid) { return grid ? grid->num_cells : 0; }

int gp_occupancy_grid_info(const gp_occupancy_grid_t* grid, int* num_slots, int* num_blocks) {
  if (!grid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_occupancy_grid_info: grid is NULL");
  if (num_slots) *num_slots = (int)grid->slots;
  if (num_blocks) *num_blocks = grid->num_blocks;
  return GP_OK;
}

}  // extern "C"
