// gp_sampling.hip -- voxelgrid_sampling / randomgrid_sampling / sample on the device (types/point_cloud_cpu.hpp:110-156, point_cloud_cpu_funcs.cpp:27-75,119-295,
// 298-456: CPU-only upstream; a device counterpart, not a port).
//
// A PLAN is built once per (cloud, resolution): the valid points sorted by voxel, the voxels numbered in ascending order of the reference's packed key
// (z << 42 | y << 21 | x of the coordinates + 2^20, :143-146), i.e. lexicographically by (z, y, x); inside a voxel the points are in ascending point index (the
// sort is stable).  Any number of attribute reductions (gp_voxelgrid_plan_average) or index selections (gp_voxelgrid_plan_random_indices) then run on it.
//   voxel coordinate  floor(double(p) * (1.0 / resolution)) per axis (:128,136), as bin_points
//   dropped points    not finite, or coordinate + 2^20 outside [0, 2^21 - 1] on some axis (:132-140): counted, in no output (the reference lumps them under one invalid
//                     key and emits a NaN row for them; that row is not reproduced)
//   one row per voxel the reference cuts its sorted array into blocks of 1024 and emits a voxel that straddles a cut once per block (:188-206): an artefact of its
//                     threading.  The device emits exactly one row per occupied voxel.
// Two sort routes, one numbering: a bounding box of at most 2^32 - 1 cells sorts ONCE on the z-major ordinal inside the box, with only as many key bits as the box
// needs; a larger box sorts twice (stable), on the low and then the high 32 bits of the 63-bit key.  The ordinal is monotone in the key, so the voxel order is the same.
// Every sort keeps the bounded-wait protocol of gp_sort.hpp: a faulted sort voids the build, which runs again with one ticket class.
#include <cmath>
#include <cstdint>

#include "gp_select.hpp"
#include "gp_sort.hpp"

struct gp_voxelgrid_plan {
  int n = 0;           // points of the cloud
  int num_valid = 0;   // points with a voxel; sorted positions [0, num_valid)
  int num_voxels = 0;
  bool wide_keys = false;  // the build took the two-sort route
  double resolution = 0.0;
  hipStream_t stream = nullptr;
  gp::DeviceArray order;        // int[n]: point index at a sorted position (valid points first, by (voxel, index))
  gp::DeviceArray voxel_of;     // int[n]: voxel of a sorted position (valid positions only)
  gp::DeviceArray voxel_start;  // int[num_voxels + 1]: first sorted position of a voxel; [num_voxels] = num_valid
};

namespace gp {
thread_local SortHooks g_voxelgrid_sort_hooks;  // (gp_sort.hpp)
namespace {

constexpr double kCoordLimit = 1048576.0;  // 2^20: a coordinate c is kept when 0 <= c + 2^20 <= 2^21 - 1, i.e. -2^20 <= u < 2^20 for c = floor(u)
constexpr int kCoordOffset = 1 << 20;
constexpr int kPointTile = 4096;  // points per workgroup of the per-point kernels (256 threads x 16)

__device__ __forceinline__ bool sample_coord(const float* __restrict__ points, size_t i, double inv, int& cx, int& cy, int& cz) {
  const double ux = (double)points[3 * i] * inv, uy = (double)points[3 * i + 1] * inv, uz = (double)points[3 * i + 2] * inv;
  const bool ok = ux >= -kCoordLimit && ux < kCoordLimit && uy >= -kCoordLimit && uy < kCoordLimit && uz >= -kCoordLimit && uz < kCoordLimit;  // false for NaN / inf
  cx = ok ? fast_floor(ux) : 0;
  cy = ok ? fast_floor(uy) : 0;
  cz = ok ? fast_floor(uz) : 0;
  return ok;
}

// bounding box of the valid points' coordinates and their number: one 32-byte record per workgroup in host-mapped memory, combined by the host (CellBox::publish and
// collect_boxes, gp_cells.hpp: the count rides in the record's extra word)
__global__ void __launch_bounds__(256) sampling_bbox_kernel(const float* __restrict__ points, int n, double inv, int* __restrict__ slots /* host-mapped */, int seq) {
  CellBox box;
  int count = 0;
  const size_t tiles = ((size_t)n + kPointTile - 1) / kPointTile;
  for (size_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
#pragma unroll 4
    for (int r = 0; r < kPointTile / 256; r++) {
      const size_t i = tile * kPointTile + (size_t)r * 256 + threadIdx.x;
      if (i >= (size_t)n) break;
      int c[3];
      if (sample_coord(points, i, inv, c[0], c[1], c[2])) {
        count++;
        box.add(c);
      }
    }
  }
  __shared__ int wave_box[4][6], wave_count[4];
  count = wave_sum(count);
  if ((threadIdx.x & 63) == 0) wave_count[threadIdx.x >> 6] = count;
  box.block_reduce(wave_box);  // (its barrier also publishes the counts)
  if (threadIdx.x == 0) box.publish(slots, wave_count[0] + wave_count[1] + wave_count[2] + wave_count[3], seq);
}

// narrow route: the z-major ordinal inside the box (< 2^32 - 1); a dropped point carries invalid_key, which is above every ordinal
__global__ void __launch_bounds__(256) sampling_key32_kernel(const float* __restrict__ points, int n, double inv, int lox, int loy, int loz, unsigned long long nx,
                                                             unsigned long long ny, unsigned* __restrict__ keys, unsigned invalid_key) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  int cx, cy, cz;
  const bool ok = sample_coord(points, i, inv, cx, cy, cz);
  keys[i] = ok ? (unsigned)(((unsigned long long)(cz - loz) * ny + (unsigned long long)(cy - loy)) * nx + (unsigned long long)(cx - lox)) : invalid_key;
}

// wide route: the reference's packed key itself (:143-146); a dropped point carries the all-ones key (a valid key has bit 63 clear)
__global__ void __launch_bounds__(256) sampling_key64_kernel(const float* __restrict__ points, int n, double inv, unsigned long long* __restrict__ key64,
                                                             unsigned* __restrict__ key_lo) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  int cx, cy, cz;
  const bool ok = sample_coord(points, i, inv, cx, cy, cz);
  const unsigned long long k =
    ok ? ((unsigned long long)(cz + kCoordOffset) << 42 | (unsigned long long)(cy + kCoordOffset) << 21 | (unsigned long long)(cx + kCoordOffset)) : ~0ull;
  key64[i] = k;
  key_lo[i] = (unsigned)k;
}
__global__ void __launch_bounds__(256) sampling_key_hi_kernel(const unsigned long long* __restrict__ key64, const int* __restrict__ order, int n, unsigned* __restrict__ key_hi) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)n) key_hi[i] = (unsigned)(key64[order[i]] >> 32);
}

// 1 where a voxel starts in the sorted order (the input of the scan that numbers the voxels)
struct HeadOfSortedKeys {
  const unsigned* keys;
  unsigned invalid_key;
  __device__ __forceinline__ int operator()(long long i) const {
    const unsigned k = keys[i];
    return k != invalid_key && (i == 0 || keys[i - 1] != k);
  }
};
struct HeadOfWideKeys {
  const unsigned long long* key64;  // by point index
  const int* order;
  __device__ __forceinline__ int operator()(long long i) const {
    const unsigned long long k = key64[order[i]];
    return k != ~0ull && (i == 0 || key64[order[i - 1]] != k);
  }
};

// scan[i] = voxels that start in front of sorted position i  ->  voxel_start[], and scan[i] becomes the voxel OF position i
template <typename Head>
__global__ void __launch_bounds__(256) sampling_voxel_start_kernel(const Head head, int n, int* __restrict__ scan, int* __restrict__ voxel_start, const int* __restrict__ total,
                                                                   int num_valid) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (size_t)n) return;
  const int f = head((long long)i), e = scan[i];
  if (f) voxel_start[e] = (int)i;  // e < number of voxels <= n
  scan[i] = e + f - 1;
  if (i == 0) voxel_start[*total] = num_valid;  // *total <= n: voxel_start has n + 1 entries
}

// the plan's last kernel: the number of voxels and the sort's fault words for the host, behind them the flag (HostWords)
__global__ void sampling_report_kernel(const int* __restrict__ total, const unsigned* __restrict__ sort_state, unsigned sort_pass_words, int sort_passes,
                                       int* __restrict__ host_words /* host-mapped */, int seq) {
  host_words[8] = *total;
  host_words[9] = sort_passes > 0 ? (int)(radix_sort_faults(sort_state, sort_pass_words, sort_passes) != 0u) : 0;
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  host_words[HostWords::kFlag] = seq;
}

// ---- the per-voxel mean: a segmented reduction over tiles of the sorted order ------------------------------------------------------------------------------------
// A workgroup takes kAvgTile consecutive sorted positions: their point indices go to LDS (coalesced), the rows are gathered through them into LDS -- consecutive
// lanes read the consecutive floats of a 4 .. 64-byte row --, and one lane per (voxel of the tile, column) adds that voxel's rows of the tile in ascending position
// in f64.  A voxel that lies inside the tile is finished there: sum / count in f64, rounded once to f32.  The (at most two) voxels that cross a tile edge leave their
// partial sums in the tile's carry record -- [0] the voxel that began in an earlier tile, [1] the voxel that begins here and goes on -- and sampling_carry_kernel adds
// them in tile order: the tile a voxel begins in owns it.  No floating-point atomics; the order of every addition is fixed by the plan alone, so a result does not
// depend on the run or on which other attributes are reduced.  Voxel populations are very uneven (hundreds of points next to the sensor, one far out): the tile bounds
// the serial chain of a lane at kAvgTile additions whatever the population.
// Bytes per point and attribute of width w: 4 (order) + 4 w (the row, gathered) + 4 (voxel_of / voxel_start, amortised) read, 4 w / population written.
constexpr int kAvgTile = 512;
template <int WT>  // compile-time width (0 = run-time: the division by the width is then a real one)
__global__ void __launch_bounds__(256) sampling_average_kernel(const float* __restrict__ attr, int width, const int* __restrict__ order, const int* __restrict__ voxel_of,
                                                               const int* __restrict__ voxel_start, int num_valid, float* __restrict__ out, double* __restrict__ carry) {
  const int W = WT ? WT : width;
  extern __shared__ float rows[];  // [kAvgTile][W]
  __shared__ int index[kAvgTile];
  const int tile = blockIdx.x, t0 = tile * kAvgTile, tn = min(kAvgTile, num_valid - t0), t1 = t0 + tn;
  for (int p = threadIdx.x; p < tn; p += 256) index[p] = order[t0 + p];
  __syncthreads();
  for (int e = threadIdx.x; e < tn * W; e += 256) {
    const int p = e / W, c = e - p * W;
    rows[e] = attr[(size_t)index[p] * W + c];
  }
  __syncthreads();
  const int v_first = voxel_of[t0], jobs = (voxel_of[t1 - 1] - v_first + 1) * W;
  for (int job = threadIdx.x; job < jobs; job += 256) {
    const int dv = job / W, c = job - dv * W, v = v_first + dv;
    const int s0 = voxel_start[v], s1 = voxel_start[v + 1];
    const int b = max(s0, t0), e = min(s1, t1);
    double sum = 0.0;
    for (int p = b; p < e; p++) sum += (double)rows[(p - t0) * W + c];
    if (s0 >= t0 && s1 <= t1) {
      out[(size_t)v * W + c] = (float)(sum / (double)(s1 - s0));
    } else {
      carry[((size_t)tile * 2 + (s0 < t0 ? 0 : 1)) * W + c] = sum;
    }
  }
}
// one lane per (tile, column): the voxel that begins in the tile and ends in a later one
__global__ void __launch_bounds__(256) sampling_carry_kernel(int width, int tiles, const int* __restrict__ voxel_of, const int* __restrict__ voxel_start, int num_valid,
                                                             const double* __restrict__ carry, float* __restrict__ out) {
  const size_t j = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= (size_t)tiles * width) return;
  const int tile = (int)(j / width), c = (int)(j - (size_t)tile * width);
  const int t0 = tile * kAvgTile, t1 = min(t0 + kAvgTile, num_valid);
  const int v = voxel_of[t1 - 1], s0 = voxel_start[v], s1 = voxel_start[v + 1];
  if (s1 <= t1 || s0 < t0) return;  // ends here, or belongs to an earlier tile
  double sum = carry[((size_t)tile * 2 + 1) * width + c];
  for (int k = tile + 1; k * kAvgTile < s1; k++) sum += carry[((size_t)k * 2) * width + c];
  out[(size_t)v * width + c] = (float)(sum / (double)(s1 - s0));
}

// out[i] = attr[indices[i]]: sample() (:27-75) for one float attribute
__global__ void __launch_bounds__(256) cloud_gather_kernel(const float* __restrict__ attr, int width, const int* __restrict__ indices, size_t elements, float* __restrict__ out) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= elements) return;
  const size_t i = e / (unsigned)width;
  out[e] = attr[(size_t)indices[i] * width + (e - i * width)];
}

// ---- randomgrid_sampling ---------------------------------------------------------------------------------------------------------------------------------------------
// counter-based: a point's rank value is a function of (seed, point index) alone -- no generator state, the same selection on every run
__host__ __device__ __forceinline__ unsigned mix32(unsigned x) {
  x ^= x >> 16;
  x *= 0x7feb352du;
  x ^= x >> 15;
  x *= 0x846ca68bu;
  x ^= x >> 16;
  return x;
}
__host__ __device__ __forceinline__ unsigned sample_hash(unsigned long long seed, unsigned index) {
  const unsigned a = mix32((unsigned)seed ^ 0x9e3779b9u);
  const unsigned b = mix32((unsigned)(seed >> 32) + 0x7f4a7c15u + a);
  return mix32(mix32(index ^ b) + a);
}

__global__ void __launch_bounds__(256) sampling_hash_positions_kernel(const int* __restrict__ order, int m, unsigned long long seed, unsigned* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)m) keys[i] = sample_hash(seed, (unsigned)order[i]);
}
__global__ void __launch_bounds__(256) sampling_voxel_keys_kernel(const int* __restrict__ positions, const int* __restrict__ voxel_of, int m, unsigned* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)m) keys[i] = (unsigned)voxel_of[positions[i]];
}
// slot s of the (voxel, hash, index)-sorted list holds the voxel's (s - voxel_start)-th smallest: kept while that rank is below points_per_voxel
__global__ void __launch_bounds__(256) sampling_mark_ranked_kernel(const unsigned* __restrict__ voxel_keys, const int* __restrict__ positions, const int* __restrict__ voxel_start,
                                                                   const int* __restrict__ order, int m, unsigned long long points_per_voxel, int* __restrict__ selected) {
  const size_t s = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (size_t)m) return;
  const unsigned long long rank = (unsigned long long)((long long)s - (long long)voxel_start[voxel_keys[s]]);
  if (rank < points_per_voxel) selected[order[positions[s]]] = 1;
}
__global__ void __launch_bounds__(256) sampling_mark_kernel(const int* __restrict__ indices, int m, int* __restrict__ selected) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)m) selected[indices[i]] = 1;
}
__global__ void __launch_bounds__(256) sampling_hash_indices_kernel(const int* __restrict__ indices, int m, unsigned long long seed, unsigned* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)m) keys[i] = sample_hash(seed, (unsigned)indices[i]);
}

thread_local int g_force_wide_keys = 0;  // test hook (gp_debug_voxelgrid_hooks)

int plan_build_once(gp_voxelgrid_plan* plan, const float* points, int classes, bool* fault) {
  *fault = false;
  const int n = plan->n;
  hipStream_t s = plan->stream;
  const double inv = 1.0 / plan->resolution;
  HostWords hw;
  HostSlots slots;
  GP_TRY(HostWords::get(&hw));
  GP_TRY(HostSlots::get(&slots));
  // ---- bounding box of the valid coordinates, and their number ----
  const int box_wgs = (int)std::min<size_t>(((size_t)n + kPointTile - 1) / kPointTile, (size_t)HostSlots::kSlots);
  const int seq_box = hw.next_seq();
  hipLaunchKernelGGL(sampling_bbox_kernel, dim3(box_wgs), dim3(256), 0, s, points, n, inv, slots.dev, seq_box);
  GP_HIP(hipGetLastError());
  PairSort ps;
  DeviceArray scan_state, total, key64;
  GP_TRY(plan->order.alloc_pooled(sizeof(int) * (size_t)n, s));
  GP_TRY(plan->voxel_of.alloc_pooled(sizeof(int) * (size_t)n, s));
  GP_TRY(plan->voxel_start.alloc_pooled(sizeof(int) * ((size_t)n + 1), s));
  GP_TRY(ps.alloc(n, s, false));
  GP_TRY(scan_state.alloc_pooled(sizeof(unsigned long long) * onepass_state_words(n), s));
  GP_TRY(total.alloc_pooled(sizeof(int), s));
  auto release_scratch = [&]() {
    ps.release_on(s), scan_state.release_on(s), total.release_on(s), key64.release_on(s);
  };
  int box[6];
  long long valid = 0;
  GP_TRY(collect_boxes(slots, box_wgs, seq_box, s, "gp_voxelgrid_plan_create", box, &valid));
  const long long lo[3] = {box[0], box[1], box[2]}, hi[3] = {box[3], box[4], box[5]};
  plan->num_valid = (int)valid;
  plan->num_voxels = 0;
  if (valid == 0) {
    release_scratch();
    return GP_OK;
  }
  const unsigned long long nx = (unsigned long long)(hi[0] - lo[0] + 1), ny = (unsigned long long)(hi[1] - lo[1] + 1), nz = (unsigned long long)(hi[2] - lo[2] + 1);  // <= 2^21 each
  const unsigned long long cells = nx * ny * nz;                                                                                                                  // <= 2^63
  plan->wide_keys = g_force_wide_keys != 0 || cells > 0xffffffffull;
  GP_HIP(hipMemsetAsync(scan_state.ptr, 0, sizeof(unsigned long long) * onepass_state_words(n), s));
  const unsigned grid = blocks_of((size_t)n);
  int sort_passes = 0;
  if (!plan->wide_keys) {
    int key_bits = 1;
    while (((1ull << key_bits) - 1ull) < cells) key_bits++;  // the all-ones key of that width is above every ordinal: <= 32 bits
    const unsigned invalid_key = (unsigned)((1ull << key_bits) - 1ull);
    hipLaunchKernelGGL(sampling_key32_kernel, dim3(grid), dim3(256), 0, s, points, n, inv, (int)lo[0], (int)lo[1], (int)lo[2], nx, ny, ps.keys_a.as<unsigned>(), invalid_key);
    GP_HIP(hipGetLastError());
    GP_TRY(ps.sort(plan->order, n, key_bits, true, s, classes));
    sort_passes = (key_bits + 7) / 8;
    // (nothing below indexes with a key or, before the host has seen the fault words, with a sorted value)
    const HeadOfSortedKeys head{ps.keys_a.as<unsigned>(), invalid_key};
    GP_TRY(exclusive_scan_of(head, plan->voxel_of.as<int>(), (long long)n, total.as<int>(), s, scan_state.as<unsigned long long>()));
    hipLaunchKernelGGL(sampling_voxel_start_kernel<HeadOfSortedKeys>, dim3(grid), dim3(256), 0, s, head, n, plan->voxel_of.as<int>(), plan->voxel_start.as<int>(),
                       (const int*)total.as<int>(), plan->num_valid);
    GP_HIP(hipGetLastError());
  } else {
    GP_TRY(key64.alloc_pooled(sizeof(unsigned long long) * (size_t)n, s));
    hipLaunchKernelGGL(sampling_key64_kernel, dim3(grid), dim3(256), 0, s, points, n, inv, key64.as<unsigned long long>(), ps.keys_a.as<unsigned>());
    GP_HIP(hipGetLastError());
    GP_TRY(ps.sort(plan->order, n, 32, true, s, classes));
    GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), n, 32, s, fault));  // (waits: the next kernel indexes with the sorted values)
    if (!*fault) {
      hipLaunchKernelGGL(sampling_key_hi_kernel, dim3(grid), dim3(256), 0, s, (const unsigned long long*)key64.as<unsigned long long>(), (const int*)plan->order.as<int>(), n,
                         ps.keys_a.as<unsigned>());
      GP_HIP(hipGetLastError());
      GP_TRY(ps.sort(plan->order, n, 32, false, s, classes < 0 ? kSortTicketClasses : classes));
      GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), n, 32, s, fault));
    }
    if (*fault) {
      release_scratch();
      return GP_OK;
    }
    const HeadOfWideKeys head{key64.as<unsigned long long>(), plan->order.as<int>()};
    GP_TRY(exclusive_scan_of(head, plan->voxel_of.as<int>(), (long long)n, total.as<int>(), s, scan_state.as<unsigned long long>()));
    hipLaunchKernelGGL(sampling_voxel_start_kernel<HeadOfWideKeys>, dim3(grid), dim3(256), 0, s, head, n, plan->voxel_of.as<int>(), plan->voxel_start.as<int>(),
                       (const int*)total.as<int>(), plan->num_valid);
    GP_HIP(hipGetLastError());
  }
  // ---- ONE wait: the number of voxels and the sort's fault words ----
  const int seq = hw.next_seq();
  hipLaunchKernelGGL(sampling_report_kernel, dim3(1), dim3(1), 0, s, (const int*)total.as<int>(), (const unsigned*)ps.state.as<unsigned>(), (unsigned)radix_sort_pass_words(n),
                     sort_passes, hw.dev, seq);
  GP_HIP(hipGetLastError());
  GP_TRY(hw.wait_flag(seq, s));
  release_scratch();
  if (reinterpret_cast<volatile int*>(hw.host)[9]) {
    *fault = true;
    return GP_OK;
  }
  plan->num_voxels = reinterpret_cast<volatile int*>(hw.host)[8];
  if (plan->num_voxels < 1 || plan->num_voxels > plan->num_valid) return fail(GP_ERROR_HIP, "gp_voxelgrid_plan_create: inconsistent voxel count");
  return GP_OK;
}

int random_indices_once(gp_voxelgrid_plan* plan, double rate, unsigned long long seed, int* indices_out, int* num_selected, int classes, bool* fault) {
  *fault = false;
  const int n = plan->n, m = plan->num_valid;
  hipStream_t s = plan->stream;
  const char* who = "gp_voxelgrid_plan_random_indices";
  DeviceArray selected;  // int[n], 0 / 1: the stored flags of the compactions below
  GP_TRY(selected.alloc_pooled(sizeof(int) * (size_t)n, s));
  GP_HIP(hipMemsetAsync(selected.ptr, 0, sizeof(int) * (size_t)n, s));
  if (rate >= 0.99) {  // every valid point (:300-303)
    hipLaunchKernelGGL(sampling_mark_kernel, dim3(blocks_of((size_t)m)), dim3(256), 0, s, (const int*)plan->order.as<int>(), m, selected.as<int>());
    GP_HIP(hipGetLastError());
    GP_TRY(select_indices(ScanArrayInput{selected.as<int>(), 1}, n, indices_out, s, num_selected, who));
    selected.release_on(s);
    return GP_OK;
  }
  const unsigned long long points_per_voxel = (unsigned long long)std::ceil((rate * (double)m) / (double)plan->num_voxels);  // :377
  const size_t max_num_points = (size_t)((double)m * rate * 1.2);                                                           // :378
  PairSort ps;
  GP_TRY(ps.alloc(std::max(m, 1), s, true));
  auto done = [&](int rc) {
    ps.release_on(s), selected.release_on(s);
    return rc;
  };
  // positions sorted by (hash, position), then stably by voxel: a voxel's points in ascending (hash, point index)
  hipLaunchKernelGGL(sampling_hash_positions_kernel, dim3(blocks_of((size_t)m)), dim3(256), 0, s, (const int*)plan->order.as<int>(), m, seed, ps.keys_a.as<unsigned>());
  GP_HIP(hipGetLastError());
  GP_TRY(ps.sort(ps.vals_a, m, 32, true, s, classes));
  GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), m, 32, s, fault));  // (waits: the kernels below index with the sorted values)
  if (*fault) return done(GP_OK);
  if (classes < 0) classes = kSortTicketClasses;
  int voxel_bits = 1;
  while ((1ll << voxel_bits) < (long long)plan->num_voxels) voxel_bits++;
  hipLaunchKernelGGL(sampling_voxel_keys_kernel, dim3(blocks_of((size_t)m)), dim3(256), 0, s, (const int*)ps.vals_a.as<int>(), (const int*)plan->voxel_of.as<int>(), m,
                     ps.keys_a.as<unsigned>());
  GP_HIP(hipGetLastError());
  GP_TRY(ps.sort(ps.vals_a, m, voxel_bits, false, s, classes));
  GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), m, voxel_bits, s, fault));
  if (*fault) return done(GP_OK);
  hipLaunchKernelGGL(sampling_mark_ranked_kernel, dim3(blocks_of((size_t)m)), dim3(256), 0, s, (const unsigned*)ps.keys_a.as<unsigned>(), (const int*)ps.vals_a.as<int>(),
                     (const int*)plan->voxel_start.as<int>(), (const int*)plan->order.as<int>(), m, points_per_voxel, selected.as<int>());
  GP_HIP(hipGetLastError());
  int count = 0;
  GP_TRY(select_indices(ScanArrayInput{selected.as<int>(), 1}, n, indices_out, s, &count, who));
  if ((size_t)count > max_num_points) {  // :445-449: keep max_num_points of them -- the smallest (hash, point index)
    const int keep = (int)max_num_points;
    hipLaunchKernelGGL(sampling_hash_indices_kernel, dim3(blocks_of((size_t)count)), dim3(256), 0, s, (const int*)indices_out, count, seed, ps.keys_a.as<unsigned>());
    GP_HIP(hipGetLastError());
    GP_HIP(hipMemcpyAsync(ps.vals_a.ptr, indices_out, sizeof(int) * (size_t)count, hipMemcpyDeviceToDevice, s));
    GP_TRY(ps.sort(ps.vals_a, count, 32, false, s, classes));
    GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), count, 32, s, fault));
    if (*fault) return done(GP_OK);
    GP_HIP(hipMemsetAsync(selected.ptr, 0, sizeof(int) * (size_t)n, s));
    if (keep > 0) {
      hipLaunchKernelGGL(sampling_mark_kernel, dim3(blocks_of((size_t)keep)), dim3(256), 0, s, (const int*)ps.vals_a.as<int>(), keep, selected.as<int>());
      GP_HIP(hipGetLastError());
    }
    GP_TRY(select_indices(ScanArrayInput{selected.as<int>(), 1}, n, indices_out, s, &count, who));
    if (count != keep) return done(fail(GP_ERROR_HIP, "gp_voxelgrid_plan_random_indices: the capped selection lost points"));
  }
  *num_selected = count;
  return done(GP_OK);
}

}  // namespace
}  // namespace gp

extern "C" {

int gp_voxelgrid_plan_create(const float* points_dev, int num_points, double resolution, gp_stream_t stream, gp_voxelgrid_plan_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_create: out is NULL");
  *out = nullptr;
  if (num_points < 0 || num_points >= (1 << 30) || (num_points > 0 && !points_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_create: bad points / num_points");
  if (!(resolution > 0.0) || !std::isfinite(resolution)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_create: the resolution must be positive and finite");
  auto* plan = new gp_voxelgrid_plan;
  plan->n = num_points;
  plan->resolution = resolution;
  plan->stream = (hipStream_t)stream;
  if (num_points > 0) {
    // (a fault: a tile of a sort waited for a workgroup that had not been started (gp_sort.hpp); the build is void and runs again with the single ticket counter)
    const int rc = gp::with_sort_fallback(gp::g_voxelgrid_sort_hooks, plan->stream, "gp_voxelgrid_plan_create",
                                          [&](int classes, bool* fault) { return gp::plan_build_once(plan, points_dev, classes, fault); });
    if (rc != GP_OK) {
      (void)hipDeviceSynchronize();
      delete plan;
      return rc;
    }
  }
  *out = plan;
  return GP_OK;
}

int gp_voxelgrid_plan_info(const gp_voxelgrid_plan_t* plan, int* num_voxels, int* num_dropped) {
  if (!plan) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_info: plan is NULL");
  if (num_voxels) *num_voxels = plan->num_voxels;
  if (num_dropped) *num_dropped = plan->n - plan->num_valid;
  return GP_OK;
}

int gp_voxelgrid_plan_average(gp_voxelgrid_plan_t* plan, const float* attr_dev, int width, float* out_dev) {
  if (!plan) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_average: plan is NULL");
  if (width < 1 || width > 16) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_average: width must be 1 .. 16");
  if ((plan->n > 0 && !attr_dev) || (plan->num_voxels > 0 && !out_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_average: NULL array");
  if (plan->num_voxels == 0) return GP_OK;
  hipStream_t s = plan->stream;
  const int tiles = (plan->num_valid + gp::kAvgTile - 1) / gp::kAvgTile;
  gp::DeviceArray carry;  // double[tiles][2][width]; only records of edge-crossing voxels are written, and only those are read
  GP_TRY(carry.alloc_pooled(sizeof(double) * 2 * (size_t)tiles * width, s));
  const size_t lds = sizeof(float) * gp::kAvgTile * (size_t)width;
  const int *order = plan->order.as<int>(), *voxel_of = plan->voxel_of.as<int>(), *voxel_start = plan->voxel_start.as<int>();
  switch (width) {
    case 1: hipLaunchKernelGGL(gp::sampling_average_kernel<1>, dim3(tiles), dim3(256), lds, s, attr_dev, width, order, voxel_of, voxel_start, plan->num_valid, out_dev, carry.as<double>()); break;
    case 3: hipLaunchKernelGGL(gp::sampling_average_kernel<3>, dim3(tiles), dim3(256), lds, s, attr_dev, width, order, voxel_of, voxel_start, plan->num_valid, out_dev, carry.as<double>()); break;
    case 9: hipLaunchKernelGGL(gp::sampling_average_kernel<9>, dim3(tiles), dim3(256), lds, s, attr_dev, width, order, voxel_of, voxel_start, plan->num_valid, out_dev, carry.as<double>()); break;
    default: hipLaunchKernelGGL(gp::sampling_average_kernel<0>, dim3(tiles), dim3(256), lds, s, attr_dev, width, order, voxel_of, voxel_start, plan->num_valid, out_dev, carry.as<double>()); break;
  }
  GP_HIP(hipGetLastError());
  if (tiles > 1) {
    hipLaunchKernelGGL(gp::sampling_carry_kernel, dim3(gp::blocks_of((size_t)tiles * width)), dim3(256), 0, s, width, tiles, voxel_of, voxel_start, plan->num_valid,
                       (const double*)carry.as<double>(), out_dev);
    GP_HIP(hipGetLastError());
  }
  carry.release_on(s);
  return GP_OK;
}

int gp_voxelgrid_plan_random_indices(gp_voxelgrid_plan_t* plan, double sampling_rate, unsigned long long seed, int* indices_out_dev, int* num_selected) {
  if (!plan || !num_selected) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_random_indices: plan / num_selected is NULL");
  if (!(sampling_rate > 0.0) || !(sampling_rate <= 1.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_random_indices: the sampling rate must lie in (0, 1]");
  if (plan->n > 0 && !indices_out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_voxelgrid_plan_random_indices: NULL array");
  *num_selected = 0;
  if (plan->num_valid == 0) return GP_OK;
  return gp::with_sort_fallback(gp::g_voxelgrid_sort_hooks, plan->stream, "gp_voxelgrid_plan_random_indices", [&](int classes, bool* fault) {
    return gp::random_indices_once(plan, sampling_rate, seed, indices_out_dev, num_selected, classes, fault);
  });
}

int gp_voxelgrid_plan_destroy(gp_voxelgrid_plan_t* plan) {
  if (!plan) return GP_OK;
  if (plan->order.ptr) (void)hipDeviceSynchronize();  // (the arrays go back to the pool for any stream to take)
  delete plan;
  return GP_OK;
}

int gp_cloud_gather(const float* attr_dev, int width, const int* indices_dev, int num_indices, float* out_dev, gp_stream_t stream) {
  if (width < 1 || width > 16) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_gather: width must be 1 .. 16");
  if (num_indices < 0 || (num_indices > 0 && (!attr_dev || !indices_dev || !out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_gather: bad arguments");
  if (num_indices == 0) return GP_OK;
  const size_t elements = (size_t)num_indices * width;
  hipLaunchKernelGGL(gp::cloud_gather_kernel, dim3(gp::blocks_of(elements)), dim3(256), 0, (hipStream_t)stream, attr_dev, width, indices_dev, elements, out_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_debug_voxelgrid_hooks(int force_wide_keys, int sort_faults) {
  gp::g_force_wide_keys = force_wide_keys;
  gp::g_voxelgrid_sort_hooks.inject = sort_faults < 0 ? 0 : sort_faults;
  return gp::g_voxelgrid_sort_hooks.fallbacks;
}
unsigned gp_debug_sample_hash(unsigned long long seed, unsigned index) { return gp::sample_hash(seed, index); }

}  // extern "C"
