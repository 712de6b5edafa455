// gp_cloud_filter.hip -- remove_outliers / filter / sort_by_time (point_cloud_cpu_funcs.cpp:459-465, 576-650; point_cloud_cpu.hpp:158-203): indices for sample()
// (gp_cloud_gather, gp_sampling.hip).  The mean neighbour distances the threshold is taken of come from gp_knn.hip.
#include <cmath>
#include <cstdint>

#include "gp_select.hpp"
#include "gp_sort.hpp"

namespace gp {
namespace {

// sum d, sum d^2 and the number of the FINITE entries of d[] (short points carry +inf), in an order fixed by n alone: a workgroup takes a tile of kStatTile entries,
// lane t its entries t, t + 256, ... in ascending order; the lanes meet in the shuffle tree and the four waves in wave order (gp_corr_factors.hip, store_tile_sums);
// one workgroup then adds the tiles' partials the same way (lane t: tiles t, t + 256, ...).  No floating-point atomics: two runs give the same bits.
constexpr int kStatTile = 4096;
__device__ __forceinline__ void stat_reduce(double sum, double sq, int count, double* __restrict__ out_sums /*[2]*/, int* __restrict__ out_count) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double lds[4][2];
  __shared__ int lds_count[4];
  sum = wave_sum(sum), sq = wave_sum(sq), count = wave_sum(count);
  if (lane == 0) lds[wave][0] = sum, lds[wave][1] = sq, lds_count[wave] = count;
  __syncthreads();
  if (threadIdx.x < 2) out_sums[threadIdx.x] = (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
  if (threadIdx.x == 2) *out_count = (lds_count[0] + lds_count[1]) + (lds_count[2] + lds_count[3]);
}
__global__ void __launch_bounds__(256) stat_tile_kernel(const double* __restrict__ values, int n, double* __restrict__ partial_sums /*[tiles][2]*/, int* __restrict__ partial_counts) {
  const size_t begin = (size_t)blockIdx.x * kStatTile, end = min(begin + (size_t)kStatTile, (size_t)n);
  double sum = 0.0, sq = 0.0;
  int count = 0;
  for (size_t i = begin + threadIdx.x; i < end; i += 256) {
    const double d = values[i];
    if (fabs(d) <= 1.7976931348623157e308) {  // (false for inf and NaN)
      sum += d;
      sq += d * d;
      count++;
    }
  }
  stat_reduce(sum, sq, count, partial_sums + 2 * (size_t)blockIdx.x, partial_counts + blockIdx.x);
}
__global__ void __launch_bounds__(256) stat_total_kernel(const double* __restrict__ partial_sums, const int* __restrict__ partial_counts, int tiles, double* __restrict__ out /*[3]*/) {
  double sum = 0.0, sq = 0.0;
  int count = 0;
  for (int t = threadIdx.x; t < tiles; t += 256) {
    sum += partial_sums[2 * (size_t)t];
    sq += partial_sums[2 * (size_t)t + 1];
    count += partial_counts[t];
  }
  __shared__ int total_count;
  stat_reduce(sum, sq, count, out, &total_count);
  __syncthreads();
  if (threadIdx.x == 0) out[2] = (double)total_count;
}

// the flags of the two compactions, as functions of the position (the scan and the scatter both evaluate them: no flag array)
struct BelowThreshold {
  const double* values;
  double thresh;
  __device__ __forceinline__ int operator()(long long i) const {
    const double v = values[i];
    return v < thresh && fabs(v) <= 1.7976931348623157e308;
  }
};
struct MaskSet {
  const unsigned char* mask;
  __device__ __forceinline__ int operator()(long long i) const { return mask[i] != 0; }
};

// a 32-bit key that is monotone in the order of the floats: -0 = +0, every NaN the largest key (NaN times go last, among themselves in ascending index)
__host__ __device__ __forceinline__ unsigned time_sort_key(unsigned bits) {
  if ((bits & 0x7fffffffu) > 0x7f800000u) return 0xffffffffu;
  if (bits == 0x80000000u) bits = 0u;
  return (bits & 0x80000000u) ? ~bits : (bits | 0x80000000u);
}
__global__ void __launch_bounds__(256) time_keys_kernel(const float* __restrict__ times, int n, unsigned* __restrict__ keys) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)n) keys[i] = time_sort_key(__float_as_uint(times[i]));
}

int sort_by_time_once(const float* times, int n, int* indices_out, hipStream_t s, int classes, bool* fault) {
  *fault = false;
  PairSort ps;
  GP_TRY(ps.alloc(n, s, false));
  hipLaunchKernelGGL(time_keys_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, s, times, n, ps.keys_a.as<unsigned>());
  GP_HIP(hipGetLastError());
  bool in_b = false;  // (the caller's array is the sort's value storage: four passes end in it)
  GP_TRY(radix_sort_pairs(ps.keys_a.as<unsigned>(), indices_out, ps.keys_b.as<unsigned>(), ps.vals_b.as<int>(), n, 32, true, ps.state.as<unsigned>(), false, false, s, &in_b, classes));
  if (in_b) GP_HIP(hipMemcpyAsync(indices_out, ps.vals_b.ptr, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), n, 32, s, fault));  // (waits)
  ps.release_on(s);
  return GP_OK;
}

int sort_indices_by_key_once(const unsigned* keys, int n, int key_bits, unsigned* sorted_keys, int* order, hipStream_t s, int classes, bool* fault) {
  *fault = false;
  PairSort ps;
  GP_TRY(ps.alloc(n, s, false));
  GP_HIP(hipMemcpyAsync(ps.keys_a.ptr, keys, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, s));  // (the passes overwrite their input; a second run needs it again)
  bool in_b = false;
  GP_TRY(radix_sort_pairs(ps.keys_a.as<unsigned>(), order, ps.keys_b.as<unsigned>(), ps.vals_b.as<int>(), n, key_bits, true, ps.state.as<unsigned>(), false, false, s, &in_b, classes));
  GP_HIP(hipMemcpyAsync(sorted_keys, in_b ? ps.keys_b.ptr : ps.keys_a.ptr, sizeof(unsigned) * (size_t)n, hipMemcpyDeviceToDevice, s));
  if (in_b) GP_HIP(hipMemcpyAsync(order, ps.vals_b.ptr, sizeof(int) * (size_t)n, hipMemcpyDeviceToDevice, s));
  GP_TRY(radix_sort_fault(ps.state.as<unsigned>(), n, key_bits, s, fault));  // (waits)
  ps.release_on(s);
  return GP_OK;
}

}  // namespace

// gp_host.hpp: the stable sort of 0 .. n - 1 by a key array, under the retry rule of every sort here (the voxel-grid plan's hooks govern this one too)
int sort_indices_by_key(const unsigned* keys_dev, int n, int key_bits, unsigned* sorted_keys_dev, int* order_dev, hipStream_t s, const char* who) {
  if (n <= 0) return GP_OK;
  return with_sort_fallback(g_voxelgrid_sort_hooks, s, who, [&](int classes, bool* fault) { return sort_indices_by_key_once(keys_dev, n, key_bits, sorted_keys_dev, order_dev, s, classes, fault); });
}
}  // namespace gp

extern "C" {

int gp_cloud_inlier_threshold(const double* mean_dists_dev, int n, double std_thresh, double* stats_host, gp_stream_t stream) {
  if (n < 0 || n >= (1 << 30) || !stats_host || (n > 0 && !mean_dists_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_inlier_threshold: bad arguments");
  if (!std::isfinite(std_thresh)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_inlier_threshold: std_thresh must be finite");
  stats_host[0] = stats_host[1] = stats_host[2] = stats_host[3] = 0.0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  const int tiles = (n + gp::kStatTile - 1) / gp::kStatTile;
  gp::DeviceArray sums, counts;  // double[tiles][2] + the three totals, int[tiles]
  GP_TRY(sums.alloc_pooled(sizeof(double) * (2 * (size_t)tiles + 4), s));
  GP_TRY(counts.alloc_pooled(sizeof(int) * (size_t)tiles, s));
  double* totals = sums.as<double>() + 2 * (size_t)tiles;
  hipLaunchKernelGGL(gp::stat_tile_kernel, dim3(tiles), dim3(256), 0, s, mean_dists_dev, n, sums.as<double>(), counts.as<int>());
  GP_HIP(hipGetLastError());
  hipLaunchKernelGGL(gp::stat_total_kernel, dim3(1), dim3(256), 0, s, (const double*)sums.as<double>(), (const int*)counts.as<int>(), tiles, totals);
  GP_HIP(hipGetLastError());
  double h[3] = {0.0, 0.0, 0.0};
  GP_HIP(hipMemcpyAsync(h, totals, sizeof(h), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  sums.release_on(s), counts.release_on(s);
  const double m = h[2];
  if (m > 0.0) {  // :598-600 with the divisor m: the one-pass variance, not clamped (a negative one gives a NaN threshold, below which nothing lies -- as upstream)
    const double mean = h[0] / m;
    const double var = h[1] / m - mean * mean;
    stats_host[0] = mean;
    stats_host[1] = var;
    stats_host[2] = mean + std::sqrt(var) * std_thresh;
  }
  stats_host[3] = m;
  return GP_OK;
}

int gp_cloud_select_below(const double* values_dev, int n, double thresh, int* indices_out_dev, int* num_selected, gp_stream_t stream) {
  if (n < 0 || n >= (1 << 30) || !num_selected || (n > 0 && (!values_dev || !indices_out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_select_below: bad arguments");
  *num_selected = 0;
  if (n == 0) return GP_OK;
  return gp::select_indices(gp::BelowThreshold{values_dev, thresh}, n, indices_out_dev, (hipStream_t)stream, num_selected, "gp_cloud_select_below");
}

int gp_cloud_select_mask(const unsigned char* mask_dev, int n, int* indices_out_dev, int* num_selected, gp_stream_t stream) {
  if (n < 0 || n >= (1 << 30) || !num_selected || (n > 0 && (!mask_dev || !indices_out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_select_mask: bad arguments");
  *num_selected = 0;
  if (n == 0) return GP_OK;
  return gp::select_indices(gp::MaskSet{mask_dev}, n, indices_out_dev, (hipStream_t)stream, num_selected, "gp_cloud_select_mask");
}

int gp_cloud_sort_by_time_indices(const float* times_dev, int n, int* indices_out_dev, gp_stream_t stream) {
  if (n < 0 || n >= (1 << 30) || (n > 0 && (!times_dev || !indices_out_dev))) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_cloud_sort_by_time_indices: bad arguments");
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;  // (a faulted sort is void and runs again with one ticket class, as gp_voxelgrid_plan_create's; its hooks govern this one too)
  return gp::with_sort_fallback(gp::g_voxelgrid_sort_hooks, s, "gp_cloud_sort_by_time_indices",
                                [&](int classes, bool* fault) { return gp::sort_by_time_once(times_dev, n, indices_out_dev, s, classes, fault); });
}

}  // extern "C"
