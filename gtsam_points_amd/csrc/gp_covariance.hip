// gp_covariance.hip -- covariance and normal estimation of a point cloud on the exact k-NN search of gp_knn_search.hpp (BASELINE.json configs[4]): one structure
// build (gp_knn.hip, point_grid_create_impl), the queries in heavy-first order, the per-lane search (covariance_kernel) beside the cooperative search of the sparse
// neighbourhoods (gp_covariance_far.hpp) on a side stream that the pipe probe picks (gp_side_stream.hip), optionally the row-tiled pass of gp_covariance_rows.hpp in
// front.  The per-point maths is gp_covariance_point.hpp on the closed-form eigen-solver of gp_eig3.hpp.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   features/covariance_estimation.cpp:18-77                          estimate_covariances      -> gp_estimate_covariances[_ex]
//   features/normal_estimation.cpp:18-55                              estimate_normals          -> gp_estimate_normals_covariances, gp_estimate_normals_from_covs
#include <algorithm>
#include <cstdio>

#include "gp_covariance_far.hpp"
#include "gp_covariance_point.hpp"
#include "gp_covariance_rows.hpp"
#include "gp_host.hpp"
#include "gp_scan.hpp"

namespace gp {

// (store_identity, gp_covariance_point.hpp: what a point without neighbours gets)
template <bool NORMALS = false>
__global__ void __launch_bounds__(256) nonfinite_identity_kernel(const float* __restrict__ points, int n, float* __restrict__ covs, int* __restrict__ num_short,
                                                                 float* __restrict__ normals = nullptr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  if (fabsf(x) < 3.0e38f && fabsf(y) < 3.0e38f && fabsf(z) < 3.0e38f) return;
  store_identity<NORMALS>(x, (!NORMALS || covs) ? covs + 9 * (size_t)i : nullptr, NORMALS ? normals + 3 * (size_t)i : nullptr);
  atomicAdd(num_short, 1);
}

// estimate_normals(points, covs, n) (features/normal_estimation.cpp:18-50): the eigenvector of the smallest eigenvalue of a GIVEN covariance (column-major; the
// lower triangle is read, as computeDirect reads it), turned by the sign rule.  One lane per point, f64 arithmetic, one rounding at the store.
__global__ void __launch_bounds__(256) normals_from_covs_kernel(const float* __restrict__ points, const float* __restrict__ covs, int n, float* __restrict__ normals) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float* c = covs + 9 * (size_t)i;
  const double c10 = (double)c[1], c20 = (double)c[2], c21 = (double)c[5];
  const double m[9] = {(double)c[0], c10, c20, c10, (double)c[4], c21, c20, c21, (double)c[8]};
  double evals[3], V[9];
  eig3_direct<true>(m, evals, V);  // (compile-time columns: no array in memory, gp_eig3.hpp)
  store_normal(V, (double)points[3 * (size_t)i], (double)points[3 * (size_t)i + 1], (double)points[3 * (size_t)i + 2], normals + 3 * (size_t)i);
}

// Heavy queries first (round 4).  A query whose own cell holds fewer than k points cannot settle in shell 0: it walks shell 1 at least -- 26 more cells, dense ones
// scanned in full until its list is full, or shell after shell of empty space in the far field -- and a wave of such queries runs 300-500 us against a mean of ~90
// (profiles/r04_c5_wavelog.txt).  In cell-sorted order those waves are scattered over the launch, and the ones that start late ARE its tail (99 % of the waves done
// at 420 us, the last at 710).  The launch therefore takes its queries through an order array: the positions of the queries with own-cell population < k first
// (ascending, so that neighbours in the list are still neighbours in space), all others behind them -- longest-processing-time-first with a per-query predictor,
// and waves whose lanes have alike work.  Same queries, same per-query search: identical results.
// (the predictor depends on the query's CELL only, so the prefix sums run over the cells -- a few 10^5 entries -- not over the points: per cell the number of its
// points when that is below k, else 0; the points of a heavy cell c go to heavy_before[c] + their rank inside the cell, the others behind all heavy ones in order)
struct HeavyCellCount {
  const int* cell_start;
  int k;
  __device__ __forceinline__ int operator()(long long c) const {
    const int size = cell_start[c + 1] - cell_start[c];
    return size < k ? size : 0;
  }
};
__global__ void __launch_bounds__(256) heavy_first_order_kernel(const int* __restrict__ cell_start, const unsigned* __restrict__ cell_of, const int* __restrict__ heavy_before,
                                                                const int* __restrict__ num_heavy, int k, int nq, int* __restrict__ order) {
  const int t = blockIdx.x * 256 + threadIdx.x;
  if (t >= nq) return;
  if (t == 0) order[nq] = nq;  // (the list's length, where covariance_kernel's todo protocol reads it)
  const int c = (int)cell_of[t];
  const int b = cell_start[c], size = cell_start[c + 1] - b, hb = heavy_before[c];
  order[size < k ? hb + (t - b) : *num_heavy + (t - hb)] = t;
}

// estimate_covariances, per-lane search (every query walks its own shells; see knn_query_bins / knn_query): the general path, and
// the second pass of the tiled kernel below for the queries it left over (todo_list != nullptr: the *todo_count positions listed)
// MIN_WAVES = 4 (k <= 10): registers capped at 128 for four waves per SIMD instead of three: 1.41 -> 1.28 ms per 1 M points (round 2).
// FULL: k == KMAX, the list is always full: straight-line insertion (TopK<KMAX, true>)
// far_list / far_count (optional): queries whose neighbourhood is sparse (knn_query_bins, `sparse`) are not searched lane by lane -- one lane walking hundreds of
// empty blocks holds its 63 neighbours for 400-600 us, the launch's tail (profiles/r05_c5_wavelog_near_first.txt) -- but appended here for covariance_far_kernel
template <int KMAX, int MIN_WAVES = 1, bool FULL = false, bool NORMALS = false>
__global__ void __launch_bounds__(128, MIN_WAVES) covariance_kernel(SearchView g, const float* __restrict__ points, int n, int k, float* __restrict__ covs,
                                                         int* __restrict__ num_short, const int* __restrict__ todo_list, const int* __restrict__ todo_count,
                                                         int* __restrict__ far_list = nullptr, int* __restrict__ far_count = nullptr, float* __restrict__ far_bound = nullptr,
                                                         const int* __restrict__ todo_begin = nullptr, float* __restrict__ normals = nullptr) {
  int t = blockIdx.x * 128 + threadIdx.x;
  if (todo_list) {  // positions [*todo_begin, *todo_count) of the list (round 5: the heavy part and the rest are two launches on two streams)
    if (todo_begin) t += *todo_begin;
    if (t >= *todo_count) return;
    t = todo_list[t];
  }
  if (t >= n) return;
  // queries are taken in the finest grid's cell-sorted order: the lanes of a wave then sit in the same or adjacent cells,
  // walk the same shells and read the same cell ranges (coherent loads, little divergence); results go to the original index
  const float4 self = g.binned ? g.bins[0].sorted[t] : g.hashed.lv[0].sorted[t];
  const int i = __float_as_int(self.w);
  const double qx = (double)self.x, qy = (double)self.y, qz = (double)self.z;
  TopK<KMAX, FULL> top;
  top.init(k, 1.7976931348623157e308);
  int2* rl = nullptr;
  if constexpr (FULL) {  // (the k = KMAX build of estimate_covariances: flat scan, see knn_query_bins)
    __shared__ int2 range_lists[kRangeCap * kRangeStride];
    static_assert(kRangeStride == 128, "one list per thread of this kernel's workgroups");
    rl = range_lists + threadIdx.x;
  }
  bool sparse = false;
  knn_query_any<KMAX, FULL, FULL>(g, qx, qy, qz, 2 * k, top, todo_list != nullptr, rl, far_list ? &sparse : nullptr);
  if (far_list) {
    // (position in the cell-sorted array and the k-th distance found so far, rounded up; one atomic per wave)
    const unsigned long long m = __ballot(sparse);
    if (m != 0ull) {
      const int lane = threadIdx.x & 63, first = __ffsll((long long)m) - 1;
      int base = 0;
      if (lane == first) base = atomicAdd(far_count, __popcll(m));
      base = __shfl(base, first, 64);
      if (sparse) {
        const int slot = base + __popcll(m & ((1ull << lane) - 1ull));
        far_list[slot] = t;
        far_bound[slot] = __double2float_ru(top.worst());
      }
    }
    if (sparse) return;
  }
  float* out = (!NORMALS || covs) ? covs + 9 * (size_t)i : nullptr;
  float* nout = NORMALS ? normals + 3 * (size_t)i : nullptr;
  if (top.count() < k) {
    atomicAdd(num_short, 1);
    store_identity<NORMALS>(self.x, out, nout);
    return;
  }
  covariance_from_neighbours<KMAX, FULL, NORMALS>(top, points, k, out, nout, qx, qy, qz);
}

}  // namespace gp

namespace {
// ---- one call, in stages: what they share, then the stages in the order estimate_covariances_impl runs them ----
// The call's arguments, the structure, and the device lists one stage leaves for the next.  Every array is allocated, written and read in the order of `s`.
struct CovCall {
  hipStream_t s;
  const float* points;
  int k;
  float *covs, *normals;
  const gp_point_grid* g;
  gp::SearchView v;
  int nq;        // queries = the cell-sorted points; non-finite points are not among them
  int* d_short;  // the call's zeroed block: [0] queries with fewer than k neighbours, [1] length of the far list, [256 B ..) the look-back state of the heavy-first scan
  gp::DeviceArray todo;          // [nq] positions + the count behind them (+ the count of heavy ones behind that, in the heavy-first order)
  gp::DeviceArray scan_buf;      // RowScanOut: kept [kTileKeep][nq] | bound [nq] | safe [nq]
  gp::DeviceArray heavy_before;  // [num_cells] heavy queries in the cells in front
  gp::DeviceArray far;           // positions (cell-sorted array) of the queries left to the cooperative kernel + their k-th distances so far
  const int* d_todo = nullptr;   // the list the per-lane search takes its queries from: null = all nq positions in order
  int *d_far = nullptr, *d_far_count = nullptr;
  float* d_far_bound = nullptr;
};

// tiled pass over the occupied cell rows of the finest level (GP_TUNE_KNN_STRUCTURE = 3); what it cannot settle is listed for the per-lane pass
template <bool NORMALS>
static int row_tiled_pass(CovCall& c) {
  const int nq = c.nq;
  GP_TRY(c.todo.alloc_async(sizeof(int) * ((size_t)nq + 1), c.s));
  GP_TRY(c.scan_buf.alloc_async(sizeof(int) * (size_t)(gp::kTileKeep + 2) * nq, c.s));
  (void)hipMemsetAsync(c.todo.as<int>() + nq, 0, sizeof(int), c.s);
  const gp::RowScanOut scan{c.scan_buf.as<int>(), reinterpret_cast<float*>(c.scan_buf.as<int>() + (size_t)gp::kTileKeep * nq),
                            reinterpret_cast<float*>(c.scan_buf.as<int>() + (size_t)(gp::kTileKeep + 1) * nq), nq};
  const gp::PointBins& bins = c.g->bin_levels[0]->bins;
  hipLaunchKernelGGL(gp::covariance_rows_kernel, dim3(16u * (unsigned)bins.num_occ_blocks), dim3(gp::kRowThreads), 0, c.s, c.v.bins[0], (const int*)bins.occ_blocks.as<int>(), scan, 0);
  hipLaunchKernelGGL((gp::covariance_settle_kernel<10, NORMALS>), dim3((nq + 127) / 128), dim3(128), 0, c.s, c.v.bins[0].sorted, scan, c.points, c.k, c.covs, c.todo.as<int>(),
                     c.todo.as<int>() + nq, c.normals);
  c.d_todo = c.todo.as<int>();
  return GP_OK;
}

// heavy queries first (HeavyCellCount above): order[] = positions with own-cell population < k, then the rest; one scan over the cells + one scatter
static int heavy_first_order(CovCall& c) {
  const gp::PointBins& bins = c.g->bin_levels[0]->bins;
  const int nq = c.nq, nc = bins.num_cells;
  GP_TRY(c.todo.alloc_async(sizeof(int) * ((size_t)nq + 2), c.s));
  GP_TRY(c.heavy_before.alloc_async(sizeof(int) * (size_t)nc, c.s));
  int* d_heavy = c.todo.as<int>() + nq + 1;
  GP_TRY(gp::exclusive_scan_of(gp::HeavyCellCount{bins.cell_start.as<int>(), c.k}, c.heavy_before.as<int>(), nc, d_heavy, c.s,
                               reinterpret_cast<unsigned long long*>(reinterpret_cast<char*>(c.d_short) + 256)));
  hipLaunchKernelGGL(gp::heavy_first_order_kernel, dim3((nq + 255) / 256), dim3(256), 0, c.s, (const int*)bins.cell_start.as<int>(), (const unsigned*)bins.cell_of.as<unsigned>(),
                     (const int*)c.heavy_before.as<int>(), (const int*)d_heavy, c.k, nq, c.todo.as<int>());
  c.d_todo = c.todo.as<int>();
  return GP_OK;
}

// the list of the queries the per-lane search leaves to covariance_far_kernel; its length is word 1 of the zeroed block
static int far_list_alloc(CovCall& c) {
  GP_TRY(c.far.alloc_async((sizeof(int) + sizeof(float)) * (size_t)c.nq, c.s));
  c.d_far = c.far.as<int>(), c.d_far_bound = reinterpret_cast<float*>(c.far.as<int>() + c.nq), c.d_far_count = c.d_short + 1;
  return GP_OK;
}

// The build of covariance_kernel for a list length.  k <= 10 runs at four waves per SIMD: registers capped at 128 (uncapped, three waves: 1.41 vs 1.28 ms, round 2;
// capped at 96 for five waves: 41 spilled, 1.08 vs 1.07 ms -- no gain).  k = 10: the straight-line insertion of full lists (profiles/r03_c5_straightline.txt).
using CovarianceKernel = void (*)(gp::SearchView, const float*, int, int, float*, int*, const int*, const int*, int*, int*, float*, const int*, float*);
template <bool NORMALS>
static CovarianceKernel covariance_kernel_for(int k) {
  if (k == 10) return gp::covariance_kernel<10, 4, true, NORMALS>;
  if (k <= 10) return gp::covariance_kernel<10, 4, false, NORMALS>;
  return gp::covariance_kernel<32, 1, false, NORMALS>;
}

// the search launches: the per-lane search over the list (or over all positions), the cooperative kernel behind it where a far list was set up
template <bool NORMALS>
static void launch_searches(CovCall& c) {
  const int nq = c.nq;
  hipStream_t s = c.s;
  const CovarianceKernel kernel = covariance_kernel_for<NORMALS>(c.k);
  // positions [*begin, *count) of the list on stream `on`; defer: sparse neighbourhoods go to the far list instead of being searched lane by lane
  auto launch_lanes = [&](hipStream_t on, const int* count, bool defer, const int* begin) {
    hipLaunchKernelGGL(kernel, dim3((nq + 127) / 128), dim3(128), 0, on, c.v, c.points, nq, c.k, c.covs, c.d_short, c.d_todo, count, defer ? c.d_far : nullptr,
                       defer ? c.d_far_count : nullptr, defer ? c.d_far_bound : nullptr, begin, c.normals);
  };
  auto launch_far = [&] {
    // a fixed grid (the count stays on the device): one wave = four queries per workgroup, every group of 16 lanes takes queries w, w + groups, ... of the list
    const unsigned far_wgs = (unsigned)std::min<long long>(((long long)nq + 3) / 4, 8192);
    hipLaunchKernelGGL((gp::covariance_far_kernel<10, NORMALS>), dim3(far_wgs), dim3(64), 0, s, c.v.bins[0], c.points, c.k, c.covs, c.d_short, (const int*)c.d_far,
                       (const float*)c.d_far_bound, (const int*)c.d_far_count, c.normals);
  };
  const int* d_count = c.d_todo ? c.d_todo + nq : nullptr;
  gp::SideStreamHandles side;
  if (c.d_far && c.k == 10 && gp::side_stream_for(s, &side) == GP_OK) {
    // Round 5: TWO launches of the same kernel on two streams.  The heavy part of the order (own-cell population < k: the only queries that can turn out sparse)
    // runs on `s` with the deferral, covariance_far_kernel behind it; the rest runs beside it on a side stream.  The far kernel is a few hundred waves bound by
    // the latency of its round trips (150-200 us for 0.15 % of the queries): behind ONE launch it would be added to the call, here it runs under the other
    // launch's waves.  Both cover the whole order with their grids and leave by the counts on the device (the split is not known to the host).
    const int* d_heavy = c.d_todo + nq + 1;
    const bool forked = hipEventRecord(side.fork, s) == hipSuccess && hipStreamWaitEvent(side.stream, side.fork, 0) == hipSuccess;
    launch_lanes(s, d_heavy, true, nullptr);
    launch_lanes(forked ? side.stream : s, d_count, false, d_heavy);
    launch_far();
    if (forked && (hipEventRecord(side.join, side.stream) != hipSuccess || hipStreamWaitEvent(s, side.join, 0) != hipSuccess)) {
      (void)hipStreamSynchronize(side.stream);  // (the join could not be queued: wait for the side stream here, the call is synchronous anyway)
    }
  } else {
    launch_lanes(s, d_count, true, nullptr);
    if (c.d_far) launch_far();
  }
}

// the count of short queries comes back through a host-mapped word, behind a one-thread kernel whose flag the host polls (a D2H copy is a copy kernel + the
// stream synchronisation's wake-up: ~10 us more).  Waits for everything the call put on `s`.
static int short_count_to_host(hipStream_t s, const int* d_short, int* num_short) {
  int h_short = 0;
  gp::HostWords hw;
  int rc = gp::HostWords::get(&hw);
  if (rc == GP_OK) rc = hw.finish(s, d_short, 13);
  if (rc == GP_OK) {
    h_short = reinterpret_cast<volatile int*>(hw.host)[13];
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) rc = gp::hip_fail(e, "covariance_kernel", __FILE__, __LINE__);
  }
  if (num_short) *num_short = h_short;
  if (h_short > 0) fprintf(stderr, "warning: fewer than k neighbors found for %d points\n", h_short);  // covariance_estimation.cpp:28
  return rc;
}

// One search, the covariances (NORMALS = false: gp_estimate_covariances, the kernels as they always were) or the normals and / or the covariances (NORMALS = true:
// gp_estimate_normals_covariances; covs_dev may be null).  The flag is a template parameter of every kernel behind it: the covariance call keeps its registers.
template <bool NORMALS>
static int estimate_covariances_impl(const float* points_dev, int n, int k, double cell_size, float* covs_dev, float* normals_dev, int* num_short, int structure,
                                     unsigned long long* counters_dev, gp_stream_t stream) {
  if (num_short) *num_short = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  gp_point_grid_t* g = nullptr;
  // one zeroed block: [0] the count of queries with fewer than k neighbours, [256 B ..) the look-back state of the heavy-first scan (sized for one cell per point).
  // It is zeroed by one of the structure build's kernels on its way (gp_host.hpp, FillJob); only the hashed fallback build leaves it to a fill here.
  gp::DeviceArray d_short;
  const size_t zero_bytes = 256 + ((sizeof(unsigned long long) * gp::onepass_state_words(n) + 255) & ~size_t(255));
  GP_TRY(d_short.alloc_async(zero_bytes, s));
  bool zeroed = false;
  GP_TRY(gp::point_grid_create_impl(points_dev, n, cell_size > 0.0 ? cell_size : 0.25, structure, counters_dev, stream, true, false, &g, gp::fill_job(d_short.ptr, zero_bytes, 0u), &zeroed));
  const bool tiled = g->binned && g->structure == 3 && k <= 10;
  const bool heavy_first = g->binned && g->structure != 6 && g->structure != 3 && !g->bin_levels.empty() && g->bin_levels[0]->bins.cell_of.ptr;
  // round 5: sparse neighbourhoods are handed to covariance_far_kernel (one wave per query); structure 7 = round 4's search (every query lane by lane) for the A/B
  const bool coop_far = heavy_first && g->structure == 0 && g->bin_levels.size() == 1 && k <= 10;
  int rc = GP_OK;
  {
    if (!zeroed) (void)hipMemsetAsync(d_short.ptr, 0, zero_bytes, s);
    CovCall c{s, points_dev, k, covs_dev, normals_dev, g, g->view(), g->binned ? g->num_binned : n, d_short.as<int>()};
    if (c.nq < n) hipLaunchKernelGGL(gp::nonfinite_identity_kernel<NORMALS>, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, n, covs_dev, c.d_short, normals_dev);
    if (c.nq > 0) {
      if (tiled) rc = row_tiled_pass<NORMALS>(c);
      if (rc == GP_OK && heavy_first && !c.d_todo) rc = heavy_first_order(c);
      if (rc == GP_OK && coop_far) rc = far_list_alloc(c);
      if (rc == GP_OK) launch_searches<NORMALS>(c);
    }
    const int frc = short_count_to_host(s, c.d_short, num_short);
    if (rc == GP_OK) rc = frc;
  }
  // the structure was built and searched on `s` only, and `s` has been synchronised: its arrays go back to the pool in stream order
  // (gp_point_grid_destroy has to assume searches on other streams and synchronises the device: 1.4 ms in a process with many streams)
  g->release_on(s);
  delete g;
  return rc;
}
}  // namespace

extern "C" {

int gp_estimate_covariances(const float* points_dev, int n, int k, double cell_size, float* covs_dev, int* num_short, gp_stream_t stream) {
  return gp_estimate_covariances_ex(points_dev, n, k, cell_size, covs_dev, num_short, 0, nullptr, stream);
}

int gp_estimate_covariances_ex(const float* points_dev, int n, int k, double cell_size, float* covs_dev, int* num_short, int structure, unsigned long long* counters_dev,
                               gp_stream_t stream) {
  if (!points_dev || n < 0 || k <= 0 || k > 32 || !covs_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_covariances: bad arguments (1 <= k <= 32)");
  return estimate_covariances_impl<false>(points_dev, n, k, cell_size, covs_dev, nullptr, num_short, structure, counters_dev, stream);
}

int gp_estimate_normals_covariances(const float* points_dev, int n, int k, double cell_size, float* normals_dev, float* covs_dev, int* num_short, gp_stream_t stream) {
  if (!points_dev || n < 0 || k <= 0 || k > 32 || (!normals_dev && !covs_dev))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_normals_covariances: bad arguments (1 <= k <= 32, normals_dev and covs_dev not both null)");
  if (!normals_dev) return estimate_covariances_impl<false>(points_dev, n, k, cell_size, covs_dev, nullptr, num_short, 0, nullptr, stream);
  return estimate_covariances_impl<true>(points_dev, n, k, cell_size, covs_dev, normals_dev, num_short, 0, nullptr, stream);
}

// estimate_normals(points, covs, n) (features/normal_estimation.cpp:18-50): one lane per point, 48 B in and 12 B out
int gp_estimate_normals_from_covs(const float* points_dev, const float* covs_dev, int n, float* normals_dev, gp_stream_t stream) {
  if (!points_dev || !covs_dev || !normals_dev || n < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_normals_from_covs: bad arguments");
  if (n == 0) return GP_OK;
  hipLaunchKernelGGL(gp::normals_from_covs_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, points_dev, covs_dev, n, normals_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // extern "C"
