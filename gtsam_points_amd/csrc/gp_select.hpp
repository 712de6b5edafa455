// gp_select.hpp -- what the voxel-grid plan (gp_sampling.hip), the cloud filters (gp_cloud_filter.hip) and the correspondences of gp_gnc.hip share: THE compaction of
// all three -- flags -> exclusive scan -> scatter to ascending indices, the count to the host in one wait.  (Only the scan is needed here: a unit that sorts includes
// gp_sort.hpp itself.)
#pragma once

#include "gp_scan.hpp"

namespace gp {

// the flag is a function of the position that the scan and the scatter both evaluate: a stored array (ScanArrayInput, gp_scan.hpp), or computed from other arrays
template <typename Flag>
__global__ void __launch_bounds__(256) select_scatter_kernel(const Flag flag, const int* __restrict__ scan, int n, int* __restrict__ indices_out) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i < (size_t)n && flag((long long)i)) indices_out[scan[i]] = (int)i;  // scan[i] < number of selected entries <= n
}

// flags -> exclusive scan -> scatter: the selected positions in ascending order; *count on the host (one wait)
template <typename Flag>
int select_indices(const Flag& flag, int n, int* indices_out, hipStream_t s, int* count, const char* who) {
  DeviceArray scan, state, total;
  GP_TRY(scan.alloc_pooled(sizeof(int) * (size_t)n, s));
  GP_TRY(state.alloc_pooled(sizeof(unsigned long long) * onepass_state_words(n), s));
  GP_TRY(total.alloc_pooled(sizeof(int), s));
  GP_HIP(hipMemsetAsync(state.ptr, 0, sizeof(unsigned long long) * onepass_state_words(n), s));
  GP_TRY(exclusive_scan_of(flag, scan.as<int>(), (long long)n, total.as<int>(), s, state.as<unsigned long long>()));
  hipLaunchKernelGGL(select_scatter_kernel<Flag>, dim3(blocks_of((size_t)n)), dim3(256), 0, s, flag, (const int*)scan.as<int>(), n, indices_out);
  GP_HIP(hipGetLastError());
  HostWords hw;
  GP_TRY(HostWords::get(&hw));
  GP_TRY(hw.finish(s, total.as<int>(), 8));
  *count = reinterpret_cast<volatile int*>(hw.host)[8];
  scan.release_on(s), state.release_on(s), total.release_on(s);
  if (*count < 0 || *count > n) return fail(GP_ERROR_HIP, std::string(who) + ": inconsistent selection count");
  return GP_OK;
}

}  // namespace gp
