// gp_covariance.hip -- covariance and normal estimation of a point cloud on the exact k-NN search of gp_knn_search.hpp (BASELINE.json configs[4]): one structure
// build (gp_knn.hip, point_grid_create_impl), the queries in heavy-first order, the per-lane search (covariance_kernel) beside the cooperative search of the sparse
// neighbourhoods (covariance_far_kernel) on a side stream that the pipe probe picks, optionally the row-tiled pass of gp_covariance_rows.hpp in front.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   features/covariance_estimation.cpp:18-77                          estimate_covariances      -> gp_estimate_covariances[_ex]
//   features/normal_estimation.cpp:18-55                              estimate_normals          -> gp_estimate_normals_covariances, gp_estimate_normals_from_covs
#include <algorithm>
#include <cstdio>
#include <type_traits>

#include "gp_host.hpp"
#include "gp_knn_search.hpp"
#include "gp_scan.hpp"

namespace gp {

// non-finite points have no neighbours: identity covariance, counted as "short" (covariance_estimation.cpp:27-31)
// NORMALS (estimate_normals, features/normal_estimation.cpp:18-50): the identity's eigenbasis is the identity (computeDirect's triple root), so the normal is
// (1, 0, 0), turned round when p . n = p.x > 1 (:26).  covs may be null then (the normals-only call).
template <bool NORMALS>
__device__ __forceinline__ void store_identity(float qx, float* __restrict__ cov_out, float* __restrict__ normal_out) {
  if constexpr (NORMALS) {
    normal_out[0] = qx > 1.0f ? -1.0f : 1.0f;
    normal_out[1] = 0.0f;
    normal_out[2] = 0.0f;
    if (!cov_out) return;
  }
  for (int j = 0; j < 9; j++) cov_out[j] = (j % 4 == 0) ? 1.0f : 0.0f;
}

template <bool NORMALS = false>
__global__ void __launch_bounds__(256) nonfinite_identity_kernel(const float* __restrict__ points, int n, float* __restrict__ covs, int* __restrict__ num_short,
                                                                 float* __restrict__ normals = nullptr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const float x = points[3 * (size_t)i], y = points[3 * (size_t)i + 1], z = points[3 * (size_t)i + 2];
  if (fabsf(x) < 3.0e38f && fabsf(y) < 3.0e38f && fabsf(z) < 3.0e38f) return;
  if constexpr (NORMALS) {
    store_identity<true>(x, covs ? covs + 9 * (size_t)i : nullptr, normals + 3 * (size_t)i);
  } else {
    for (int j = 0; j < 9; j++) covs[9 * (size_t)i + j] = (j % 4 == 0) ? 1.0f : 0.0f;
  }
  atomicAdd(num_short, 1);
}

// ---- Eigen 3.4.0 SelfAdjointEigenSolver<Matrix3d>::computeDirect, restated from the published closed-form algorithm -----
__device__ __forceinline__ void eig3_roots(const double* m /*col-major sym*/, double* roots) {
  const double s_inv3 = 1.0 / 3.0, s_sqrt3 = 1.7320508075688772;
  const double c0 = m[0] * m[4] * m[8] + 2.0 * m[1] * m[2] * m[5] - m[0] * m[5] * m[5] - m[4] * m[2] * m[2] - m[8] * m[1] * m[1];
  const double c1 = m[0] * m[4] - m[1] * m[1] + m[0] * m[8] - m[2] * m[2] + m[4] * m[8] - m[5] * m[5];
  const double c2 = m[0] + m[4] + m[8];
  const double c2_over_3 = c2 * s_inv3;
  double a_over_3 = (c2 * c2_over_3 - c1) * s_inv3;
  a_over_3 = a_over_3 < 0.0 ? 0.0 : a_over_3;
  const double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
  double q = a_over_3 * a_over_3 * a_over_3 - half_b * half_b;
  q = q < 0.0 ? 0.0 : q;
  const double rho = sqrt(a_over_3);
  const double theta = atan2(sqrt(q), half_b) * s_inv3;
  const double cos_theta = cos(theta), sin_theta = sin(theta);
  roots[0] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
  roots[1] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
  roots[2] = c2_over_3 + 2.0 * rho * cos_theta;
}

__device__ __forceinline__ void eig3_extract_kernel(const double* mat, double* res, double* representative) {
  int i0 = 0;
  double best = fabs(mat[0]);
  if (fabs(mat[4]) > best) {
    best = fabs(mat[4]);
    i0 = 1;
  }
  if (fabs(mat[8]) > best) i0 = 2;
  for (int r = 0; r < 3; r++) representative[r] = mat[i0 * 3 + r];
  const int i1 = (i0 + 1) % 3, i2 = (i0 + 2) % 3;
  const double* a = representative;
  const double* b1 = mat + 3 * i1;
  const double* b2 = mat + 3 * i2;
  const double c0[3] = {a[1] * b1[2] - a[2] * b1[1], a[2] * b1[0] - a[0] * b1[2], a[0] * b1[1] - a[1] * b1[0]};
  const double c1[3] = {a[1] * b2[2] - a[2] * b2[1], a[2] * b2[0] - a[0] * b2[2], a[0] * b2[1] - a[1] * b2[0]};
  const double n0 = c0[0] * c0[0] + c0[1] * c0[1] + c0[2] * c0[2], n1 = c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2];
  if (n0 > n1) {
    const double s = 1.0 / sqrt(n0);
    for (int r = 0; r < 3; r++) res[r] = c0[r] * s;
  } else {
    const double s = 1.0 / sqrt(n1);
    for (int r = 0; r < 3; r++) res[r] = c1[r] * s;
  }
}

// STATIC_COLUMNS: the column logic a second time, with COMPILE-TIME column numbers (k, l) = (2, 0) or (0, 2).  The default indexes evecs with run-time k / l,
// which sends the array to memory: the search kernels hold it in the scratch they have anyway, but a kernel with none of its own (normals_from_covs_kernel)
// would get 72 B per lane of LDS for it.  A second copy rather than one shared form: routing the default through the shared form changes the register
// allocation of the shipped covariance kernels, which are held to their figures.
template <bool STATIC_COLUMNS = false>
__device__ __forceinline__ void eig3_direct(const double* mat /*col-major, lower triangle referenced*/, double* evals, double* evecs) {
  const double eps = 2.220446049250313e-16;
  const double shift = (mat[0] + mat[4] + mat[8]) / 3.0;
  double scaled[9] = {mat[0] - shift, mat[1], mat[2], mat[1], mat[4] - shift, mat[5], mat[2], mat[5], mat[8] - shift};
  double scale = 0.0;
  for (int i = 0; i < 9; i++) scale = fmax(scale, fabs(scaled[i]));
  if (scale > 0.0)
    for (int i = 0; i < 9; i++) scaled[i] /= scale;
  eig3_roots(scaled, evals);
  if ((evals[2] - evals[0]) <= eps) {
    for (int i = 0; i < 9; i++) evecs[i] = (i % 4 == 0) ? 1.0 : 0.0;
  } else {
    if constexpr (STATIC_COLUMNS) {
      double tmp[9];
      for (int i = 0; i < 9; i++) tmp[i] = scaled[i];
      const double d0 = evals[2] - evals[1], d1 = evals[1] - evals[0];
      auto columns = [&](auto k, auto l, double d0) {  // (k, l: std::integral_constant)
        tmp[0] -= evals[k];
        tmp[4] -= evals[k];
        tmp[8] -= evals[k];
        eig3_extract_kernel(tmp, evecs + 3 * k, evecs + 3 * l);
        if (d0 <= 2.0 * eps * d1) {
          double* ck = evecs + 3 * k;
          double* cl = evecs + 3 * l;
          const double dot = ck[0] * cl[0] + ck[1] * cl[1] + ck[2] * cl[2];
          for (int r = 0; r < 3; r++) cl[r] -= dot * cl[r];
          const double nn = sqrt(cl[0] * cl[0] + cl[1] * cl[1] + cl[2] * cl[2]);
          for (int r = 0; r < 3; r++) cl[r] /= nn;
        } else {
          double dummy[3];
          for (int i = 0; i < 9; i++) tmp[i] = scaled[i];
          tmp[0] -= evals[l];
          tmp[4] -= evals[l];
          tmp[8] -= evals[l];
          eig3_extract_kernel(tmp, evecs + 3 * l, dummy);
        }
      };
      if (d0 > d1)
        columns(std::integral_constant<int, 2>{}, std::integral_constant<int, 0>{}, d1);
      else
        columns(std::integral_constant<int, 0>{}, std::integral_constant<int, 2>{}, d0);
    } else {
      double tmp[9];
      for (int i = 0; i < 9; i++) tmp[i] = scaled[i];
      double d0 = evals[2] - evals[1];
      const double d1 = evals[1] - evals[0];
      int k = 0, l = 2;
      if (d0 > d1) {
        k = 2;
        l = 0;
        d0 = d1;
      }
      tmp[0] -= evals[k];
      tmp[4] -= evals[k];
      tmp[8] -= evals[k];
      eig3_extract_kernel(tmp, evecs + 3 * k, evecs + 3 * l);
      if (d0 <= 2.0 * eps * d1) {
        double* ck = evecs + 3 * k;
        double* cl = evecs + 3 * l;
        const double dot = ck[0] * cl[0] + ck[1] * cl[1] + ck[2] * cl[2];
        for (int r = 0; r < 3; r++) cl[r] -= dot * cl[r];
        const double nn = sqrt(cl[0] * cl[0] + cl[1] * cl[1] + cl[2] * cl[2]);
        for (int r = 0; r < 3; r++) cl[r] /= nn;
      } else {
        double dummy[3];
        for (int i = 0; i < 9; i++) tmp[i] = scaled[i];
        tmp[0] -= evals[l];
        tmp[4] -= evals[l];
        tmp[8] -= evals[l];
        eig3_extract_kernel(tmp, evecs + 3 * l, dummy);
      }
    }
    const double* c2 = evecs + 6;
    const double* c0 = evecs;
    const double c1[3] = {c2[1] * c0[2] - c2[2] * c0[1], c2[2] * c0[0] - c2[0] * c0[2], c2[0] * c0[1] - c2[1] * c0[0]};
    const double nn = sqrt(c1[0] * c1[0] + c1[1] * c1[1] + c1[2] * c1[2]);
    for (int r = 0; r < 3; r++) evecs[3 + r] = c1[r] / nn;
  }
  for (int i = 0; i < 3; i++) evals[i] = evals[i] * scale + shift;
}

__device__ __forceinline__ void inverse3_general(const double* a /*col-major*/, double* inv) {
  auto A = [&](int r, int c) { return a[c * 3 + r]; };
  const double c00 = A(1, 1) * A(2, 2) - A(1, 2) * A(2, 1), c10 = A(1, 2) * A(2, 0) - A(1, 0) * A(2, 2), c20 = A(1, 0) * A(2, 1) - A(1, 1) * A(2, 0);
  const double invdet = 1.0 / (A(0, 0) * c00 + A(0, 1) * c10 + A(0, 2) * c20);
  inv[0] = c00 * invdet;
  inv[1] = c10 * invdet;
  inv[2] = c20 * invdet;
  inv[3] = (A(0, 2) * A(2, 1) - A(0, 1) * A(2, 2)) * invdet;
  inv[4] = (A(0, 0) * A(2, 2) - A(0, 2) * A(2, 0)) * invdet;
  inv[5] = (A(0, 1) * A(2, 0) - A(0, 0) * A(2, 1)) * invdet;
  inv[6] = (A(0, 1) * A(1, 2) - A(0, 2) * A(1, 1)) * invdet;
  inv[7] = (A(0, 2) * A(1, 0) - A(0, 0) * A(1, 2)) * invdet;
  inv[8] = (A(0, 0) * A(1, 1) - A(0, 1) * A(1, 0)) * invdet;
}

// estimate_covariances (features/covariance_estimation.cpp:18-77): k-NN (query included) -> sample covariance ->
// V diag(1e-3, 1, 1) V^-1.  Fewer than k neighbours -> identity (:27-31).
// sample covariance of the k neighbours -> V diag(1e-3, 1, 1) V^-1 (features/covariance_estimation.cpp:33-53)
// NORMALS: the first eigenvector IS estimate_normals(points, n, k)'s normal (features/normal_estimation.cpp:52-55: the eigenvector of the smallest eigenvalue of
// V diag(1e-3, 1, 1) V^-1 is V's first column), stored beside the covariance, or instead of it when out == nullptr (then no inverse and no V L V^-1 products)
__device__ __forceinline__ void store_normal(const double* v, double qx, double qy, double qz, float* __restrict__ normal_out) {
  const bool away = qx * v[0] + qy * v[1] + qz * v[2] > 1.0;  // :26, points in the sensor frame
  normal_out[0] = (float)(away ? -v[0] : v[0]);
  normal_out[1] = (float)(away ? -v[1] : v[1]);
  normal_out[2] = (float)(away ? -v[2] : v[2]);
}

template <int KMAX, bool FULL, bool NORMALS = false>
__device__ __forceinline__ void covariance_from_neighbours(const TopK<KMAX, FULL>& top, const float* __restrict__ points, int k, float* __restrict__ out,
                                                           float* __restrict__ normal_out = nullptr, double qx = 0.0, double qy = 0.0, double qz = 0.0) {
  double sp[3] = {0, 0, 0}, spp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < KMAX; j++)
    if (j < k) {
      const size_t nb = (size_t)top.idx[j];
      const double p[3] = {(double)points[3 * nb], (double)points[3 * nb + 1], (double)points[3 * nb + 2]};
      for (int r = 0; r < 3; r++) sp[r] += p[r];
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) spp[c * 3 + r] += p[r] * p[c];
    }
  double cov[9];
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) cov[c * 3 + r] = (spp[c * 3 + r] - (sp[r] / (double)k) * sp[c]) / (double)k;  // :43
  double evals[3], V[9], Vinv[9];
  eig3_direct(cov, evals, V);
  if constexpr (NORMALS) {
    store_normal(V, qx, qy, qz, normal_out);
    if (!out) return;
  }
  inverse3_general(V, Vinv);
  const double lam[3] = {1e-3, 1.0, 1.0};
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) {
      double s = 0.0;
      for (int kk = 0; kk < 3; kk++) s += V[kk * 3 + r] * lam[kk] * Vinv[c * 3 + kk];
      out[c * 3 + r] = (float)s;
    }
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
  eig3_direct<true>(m, evals, V);
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

// ---- sparse neighbourhoods: SIXTEEN LANES PER QUERY (round 5) ----------------------------------------------------------------------
// A query the fine shells do not settle (the far field of a LiDAR scan: ring spacing of a metre, one point per 0.25 m cell) used to go on lane by lane: blocks as cells,
// then superblocks -- a chain of dependent loads on ONE lane while 63 wait: 400-600 us per wave against a mean of 110 (profiles/r05_c5_wavelog.txt), the tail of the
// launch.  Here kFarLanes lanes share one query (four queries per wave).  Such queries are few (0.1-1.5 % of a cloud), so the kernel runs at a fraction of a wave per
// SIMD and nothing hides a load's latency: what counts is the NUMBER OF DEPENDENT ROUND TRIPS, and every stage asks for everything it needs at once.
//   blocks -> candidates (far_process): a list of <= 128 blocks (4 x 4 x 4 cells: 1 m for the covariance structure), eight per lane: the eight block entries in one
//            trip, the sixteen cell_start words in the next, the (first point, length) ranges into LDS; then the CANDIDATES -- not the blocks -- are dealt to the lanes
//            (candidate o of the concatenated ranges to lane o % 16: one dense block does not leave fifteen lanes idle), eight loads in flight per lane;
//   phase A  the 5 x 5 x 5 blocks around the query's block: one list;
//   phase B  cube shells of SUPERBLOCKS (4 x 4 x 4 blocks, one 64-bit occupancy mask each) around the query's superblock, the masks dealt to the lanes four at a time:
//            empty space costs one 8-byte load per 64 m^3; occupied blocks outside phase A's cube and not farther than the group's best k-th distance so far are
//            appended to the list (LDS counter), which is processed whenever it is full and at the end of the shell.
// Every lane keeps the k best of what it scanned (exact f64 distances, strict '<' like KnnResult::push).  After phase A / a shell the group is done when k of its
// candidates lie within the safe radius (R units + the distance to the nearest face of the query's own unit: every unvisited point is farther) -- the stopping rule of the
// per-lane search, counted with ballots instead of read off a merged list -- or when the grid is exhausted.  Then the group merges its lists once: k rounds of "smallest
// head" (a group-wide minimum each; ties: smaller original index), which yields the neighbours in ascending order, the order covariance_from_neighbours sums them in.
// Exact like the per-lane search: the neighbour set is the k smallest distances either way.
constexpr int kFarBlockShells = 2, kFarLanes = 16, kFarList = 128, kFarPer = kFarList / kFarLanes, kFarMasks = 4;
struct FarGroupLds {
  int2 range[kFarList];  // (first point, points) per listed block
  int blk[kFarList];     // linear block index (phase B)
  int count;
  int pad_[3];
};
template <int KMAX, bool NORMALS = false>
// (four waves per SIMD = 128 registers, 560 B of scratch per lane: uncapped -- 256 registers, no scratch -- the kernel is 20 % faster ALONE (190 vs 240 us), but beside the
// other launch, whose waves hold a quarter of a SIMD's registers each, a 256-register wave waits until two of them on one SIMD have retired: profiles/r05_c5_summary.txt)
__global__ void __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(4, 4))) covariance_far_kernel(BinGridView g, const float* __restrict__ points, int k, float* __restrict__ covs, int* __restrict__ num_short,
                                                             const int* __restrict__ far_list, const float* __restrict__ far_bound, const int* __restrict__ far_count,
                                                             float* __restrict__ normals = nullptr) {
  constexpr int kGroups = 64 / kFarLanes;
  // these few waves are chains of dependent round trips with short bursts of arithmetic in between, and they run beside the other launch's waves (four per SIMD, busy
  // with list insertions): at equal issue priority every burst takes four times as long -- the kernel measured 350 us beside the light queries' launch, 190 alone
  __builtin_amdgcn_s_setprio(3);
  __shared__ FarGroupLds lds_all[kGroups];  // (one wave per workgroup: a 256-register wave finds a place where a four-wave workgroup waits for four at once)
  const int lane = threadIdx.x & 63, sub = lane % kFarLanes, grp = lane / kFarLanes;
  FarGroupLds& L = lds_all[grp];
  const unsigned long long gmask = ((1ull << kFarLanes) - 1ull) << (grp * kFarLanes);
  const int groups = (int)gridDim.x * kGroups, count = *far_count;
  constexpr double kInf = 1.7976931348623157e308;
  auto wave_sync = [] {  // LDS traffic of a wave is ordered; this keeps the compiler from moving LDS accesses across it
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  };
  for (int w0 = (int)blockIdx.x * kGroups; w0 < count; w0 += groups) {  // (wave-uniform trip count; a group without a query idles through it)
    const int w = w0 + grp;
    const bool active = w < count;
    const int t = far_list[active ? w : w0];
    // what the per-lane search knew when it gave up: its k-th distance (rounded up; +inf when it had found fewer than k) -- nothing farther can be a neighbour, so
    // blocks beyond it are not even listed (a noise point a metre above a dense surface: without it phase A scanned 6000-8000 candidates, profiles/r05_c5_farlog.txt)
    const double known = (double)far_bound[active ? w : w0];
    double bound = known;  // nothing farther than this can be a neighbour: what the per-lane search knew, then the group's exact k-th distance after every stage
    const float4 self = g.sorted[t];
    const int i = __float_as_int(self.w);
    const double qx = (double)self.x, qy = (double)self.y, qz = (double)self.z;
    const double B = 4.0 * g.h, inv_B = 0.25 * g.inv_h;
    // block coordinates RELATIVE to the grid's first block (what the superblock masks are indexed by); the query is a point of the cloud: inside the grid
    const double ux = qx * inv_B - (double)g.geom.lo[0], uy = qy * inv_B - (double)g.geom.lo[1], uz = qz * inv_B - (double)g.geom.lo[2];
    const int c[3] = {fast_floor(ux), fast_floor(uy), fast_floor(uz)};
    const double fx = ux - (double)c[0], fy = uy - (double)c[1], fz = uz - (double)c[2];
    const double face = fmin(fmin(fmin(fx, 1.0 - fx), fmin(fy, 1.0 - fy)), fmin(fz, 1.0 - fz)) * B;
    const int dim[3] = {g.geom.dim[0], g.geom.dim[1], g.geom.dim[2]};
    const double ox = (double)g.geom.lo[0] * B, oy = (double)g.geom.lo[1] * B, oz = (double)g.geom.lo[2] * B;  // corner of block (0, 0, 0)
    TopK<KMAX, false> top;
    top.init(k, kInf);
    // the blocks listed for this group (nb <= kFarList; block index of list position j from `block_of(j)`) -> their points through the lanes' lists.
    // Wave-convergent: every lane of the wave calls it, groups without work pass nb = 0
    int fresh = 0;  // candidates the group has scanned since its lists were last merged (group-uniform)
    auto far_process = [&](int nb, auto block_of, auto block_wanted) {
      if (__builtin_amdgcn_ballot_w64(nb > 0) == 0ull) return;  // (an empty shell -- an outlier walks several: no round trips for nothing)
      int4 raw[kFarPer];
      bool wanted[kFarPer];
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const int j = sub * kFarPer + q;
        wanted[q] = j < nb && block_wanted(j);
        raw[q] = *reinterpret_cast<const int4*>(g.blocks + (wanted[q] ? block_of(j) : 0));  // (unconditional: the eight loads are in flight together)
      }
      int pb[kFarPer], pe[kFarPer];
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const unsigned long long bits = ((unsigned long long)(unsigned)raw[q].y << 32) | (unsigned long long)(unsigned)raw[q].x;
        const bool valid = wanted[q] && bits != 0ull;
        pb[q] = g.cell_start[valid ? raw[q].z : 0];
        pe[q] = valid ? g.cell_start[raw[q].z + __popcll(bits)] : pb[q];
      }
      int mine = 0;
#pragma unroll
      for (int q = 0; q < kFarPer; q++) {
        const int len = wanted[q] ? pe[q] - pb[q] : 0;
        L.range[sub * kFarPer + q] = make_int2(pb[q], len);
        mine += len;
      }
      int total = mine;
#pragma unroll
      for (int off = kFarLanes / 2; off > 0; off >>= 1) total += __shfl_xor(total, off, 64);
      wave_sync();
      fresh += total;
      // candidate o of the concatenated ranges -> lane o % kFarLanes; a lane's ordinals ascend, so its cursor over the ranges only moves forward
      int rj = 0, rc = 0;  // range under the cursor, candidates in front of it
      int2 cur = L.range[0];
      constexpr int kFarCand = 4;  // candidates in flight per lane
      for (int o = sub; __builtin_amdgcn_ballot_w64(o < total) != 0ull; o += kFarLanes * kFarCand) {
        int pp[kFarCand];
        bool ok[kFarCand];
#pragma unroll
        for (int q = 0; q < kFarCand; q++) {
          const int oq = o + q * kFarLanes;
          ok[q] = oq < total;
          if (ok[q]) {
            while (oq >= rc + cur.y) {
              rc += cur.y;
              rj++;
              cur = L.range[rj];
            }
            pp[q] = cur.x + (oq - rc);
          } else {
            pp[q] = 0;
          }
        }
        float4 v[kFarCand];
#pragma unroll
        for (int q = 0; q < kFarCand; q++) v[q] = g.sorted[pp[q]];
#pragma unroll
        for (int q = 0; q < kFarCand; q++)
          if (ok[q]) {
            const double ex = (double)v[q].x - qx, ey = (double)v[q].y - qy, ez = (double)v[q].z - qz;
            const double d2 = ex * ex + ey * ey + ez * ez;
            if (d2 <= bound) top.push(__float_as_int(v[q].w), d2);
          }
      }
      // a lane that holds k candidates bounds the group's k-th distance with its own (its list is a subset of the group's): `bound` tightens after EVERY list, without a
      // merge, and prunes the rest of the shell (the kitti scan's far kernel 230 -> 192 us; profiles/r05_c5_summary.txt item 6)
      double lane_kth = top.worst();
#pragma unroll
      for (int off = kFarLanes / 2; off > 0; off >>= 1) lane_kth = fmin(lane_kth, __shfl_xor(lane_kth, off, 64));
      bound = fmin(bound, lane_kth);
      wave_sync();  // (the list may be refilled)
    };
    // k candidates of the group within `safe`?  (a lane holds its k best: one that has k within the radius settles it alone)
    auto settled_within = [&](double safe, bool live) {
      const double safe2 = safe * safe;
      int within = 0;
#pragma unroll
      for (int j = 0; j < KMAX; j++) within += __popcll(__builtin_amdgcn_ballot_w64(live && j < k && top.idx[j] >= 0 && top.d[j] <= safe2) & gmask);
      return within >= k;
    };
    // the k smallest of the group's lists, ascending (ties: smaller index): k rounds of "smallest head", a group-wide minimum each -> fin.idx (group-uniform), the
    // group's exact k-th distance in `kth` (+inf while it holds fewer than k); returns how many there are.  ~4 us: once per shell, not per block
    int fin_i[KMAX];
    double kth = kInf;
    auto merge = [&]() -> int {
#pragma unroll
      for (int r = 0; r < KMAX; r++) fin_i[r] = -1;
      kth = kInf;
      int head = 0, n_have = 0;
#pragma unroll
      for (int r = 0; r < KMAX; r++) {
        double cur = kInf;
        int cur_i = 0x7fffffff;
#pragma unroll
        for (int j = 0; j < KMAX; j++)
          if (head == j && j < k && top.idx[j] >= 0) cur = top.d[j], cur_i = top.idx[j];
        double m = cur;
#pragma unroll
        for (int off = kFarLanes / 2; off > 0; off >>= 1) m = fmin(m, __shfl_xor(m, off, 64));
        int mi = cur == m ? cur_i : 0x7fffffff;
#pragma unroll
        for (int off = kFarLanes / 2; off > 0; off >>= 1) mi = min(mi, __shfl_xor(mi, off, 64));
        if (r < k && mi != 0x7fffffff) {
          fin_i[r] = mi;
          n_have = r + 1;
          if (r == k - 1) kth = m;
          if (cur == m && cur_i == mi) head++;  // (every candidate was scanned by exactly one lane: one winner)
        }
      }
      return n_have;
    };
    int have = 0;
    bool done = !active;
    auto box2 = [&](int bx, int by, int bz) {  // squared distance of a block's box from the query
      const double bx0 = ox + (double)bx * B, by0 = oy + (double)by * B, bz0 = oz + (double)bz * B;
      const double ddx = fmax(fmax(bx0 - qx, qx - (bx0 + B)), 0.0), ddy = fmax(fmax(by0 - qy, qy - (by0 + B)), 0.0), ddz = fmax(fmax(bz0 - qz, qz - (bz0 + B)), 0.0);
      return ddx * ddx + ddy * ddy + ddz * ddz;
    };
    // ---- phase A: the blocks around the query's block: the 3 x 3 x 3 cube, then -- with the bound that brought -- the shell around it.  One list each ----
    {
      int ra_max = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) ra_max = max(ra_max, max(c[a], dim[a] - 1 - c[a]));  // the shell that covers the grid
      static_assert((2 * kFarBlockShells + 1) * (2 * kFarBlockShells + 1) * (2 * kFarBlockShells + 1) <= kFarList, "a cube of phase A is one list");
      for (int R = 1; R <= kFarBlockShells; R++) {
        const int x0 = max(c[0] - R, 0), x1 = min(c[0] + R, dim[0] - 1), y0 = max(c[1] - R, 0), y1 = min(c[1] + R, dim[1] - 1), z0 = max(c[2] - R, 0), z1 = min(c[2] + R, dim[2] - 1);
        const int nx = x1 - x0 + 1, ny = y1 - y0 + 1, nz = z1 - z0 + 1;
        far_process(
          done ? 0 : nx * ny * nz, [&](int j) { return ((size_t)(z0 + j / (nx * ny)) * (size_t)dim[1] + (size_t)(y0 + (j / nx) % ny)) * (size_t)dim[0] + (size_t)(x0 + j % nx); },
          [&](int j) {
            const int bx = x0 + j % nx, by = y0 + (j / nx) % ny, bz = z0 + j / (nx * ny);
            return (R == 1 || max(max(abs(bx - c[0]), abs(by - c[1])), abs(bz - c[2])) == R) && box2(bx, by, bz) <= bound;  // (not the cube of the step before)
          });
        const bool ok = settled_within((double)R * B + face, !done);
        if (!done && (ok || R >= ra_max)) done = true;
        if (__builtin_amdgcn_ballot_w64(!done && fresh > 0) != 0ull) {  // somebody goes on with new candidates: the exact k-th distance so far prunes what follows
          have = merge();
          bound = fmin(bound, kth);
          fresh = 0;
        }
      }
    }
    // ---- phase B: shells of superblocks (blocks outside phase A's cube) ----
    if (__builtin_amdgcn_ballot_w64(!done) != 0ull) {
      const double S = 4.0 * B;
      const int cs[3] = {c[0] >> 2, c[1] >> 2, c[2] >> 2};
      const double fsx = (ux - 4.0 * (double)cs[0]) * 0.25, fsy = (uy - 4.0 * (double)cs[1]) * 0.25, fsz = (uz - 4.0 * (double)cs[2]) * 0.25;
      const double sface = fmin(fmin(fmin(fsx, 1.0 - fsx), fmin(fsy, 1.0 - fsy)), fmin(fsz, 1.0 - fsz)) * S;
      int rs_max = 0;
#pragma unroll
      for (int a = 0; a < 3; a++) rs_max = max(rs_max, max(cs[a], g.sdim[a] - 1 - cs[a]));
      for (int R = 0; __builtin_amdgcn_ballot_w64(!done) != 0ull; R++) {  // (the wave goes on while any of its groups does; a group ends at rs_max at the latest)
        // the SURFACE of the cube of radius R, enumerated directly (an outlier tens of metres from everything walks six shells: the cube's 2197 positions at R = 6 are
        // 866 on the surface): the two z-faces, (2R + 1)^2 positions each, then 2R - 1 slabs with the 8R positions of their rim
        const int side = 2 * R + 1, face_n = side * side, rim_n = 8 * R;
        const int total = done ? 0 : (R == 0 ? 1 : 2 * face_n + (side - 2) * rim_n);
        auto shell_pos = [&](int e, int& dx, int& dy, int& dz) {
          if (R == 0) {
            dx = dy = dz = 0;
          } else if (e < 2 * face_n) {
            const int f = e / face_n, r = e % face_n;
            dz = f ? R : -R;
            dx = r % side - R;
            dy = r / side - R;
          } else {
            const int r = e - 2 * face_n, slab = r / rim_n, pos = r % rim_n, edge = pos / (2 * R), off = pos % (2 * R);
            dz = slab - R + 1;
            dx = edge == 0 ? -R + off : (edge == 1 ? R : (edge == 2 ? R - off : -R));
            dy = edge == 0 ? -R : (edge == 1 ? -R + off : (edge == 2 ? R : R - off));
          }
        };
        int e = sub;                        // next position of the shell this lane looks at (stride kFarLanes)
        unsigned long long rest[kFarMasks];  // occupied blocks of the lane's current masks that are still to be listed
        unsigned long long spos[kFarMasks];  // their superblocks, packed (x | y << 21 | z << 42: a grid has < 2^24 blocks)
#pragma unroll
        for (int q = 0; q < kFarMasks; q++) rest[q] = 0ull, spos[q] = 0;
        bool lane_more = e < total;
        while (__builtin_amdgcn_ballot_w64(lane_more) != 0ull) {  // rounds of: fill the group's list (<= kFarList blocks), process it
          // (`bound`: the group's exact k-th distance as of the last stage -- a block farther away than that holds nothing of interest)
          if (sub == 0) L.count = 0;
          wave_sync();
          bool full = false;
          while (lane_more && !full) {
            bool any_rest = false;
#pragma unroll
            for (int q = 0; q < kFarMasks; q++) any_rest = any_rest || rest[q] != 0ull;
            if (!any_rest) {  // the next kFarMasks masks of this lane's positions, requested together
              if (e >= total) {
                lane_more = false;
                break;
              }
#pragma unroll
              for (int q = 0; q < kFarMasks; q++) {
                const int eq = e + q * kFarLanes;
                int dx = 0, dy = 0, dz = 0;
                shell_pos(eq < total ? eq : 0, dx, dy, dz);
                const int x = cs[0] + dx, y = cs[1] + dy, z = cs[2] + dz;
                const bool in = eq < total && x >= 0 && x < g.sdim[0] && y >= 0 && y < g.sdim[1] && z >= 0 && z < g.sdim[2];
                const unsigned long long mask = g.super[in ? ((size_t)z * (size_t)g.sdim[1] + (size_t)y) * (size_t)g.sdim[0] + (size_t)x : 0];
                rest[q] = in ? mask : 0ull;
                spos[q] = (unsigned long long)(unsigned)x | ((unsigned long long)(unsigned)y << 21) | ((unsigned long long)(unsigned)z << 42);
              }
              e += kFarMasks * kFarLanes;
            }
#pragma unroll
            for (int q = 0; q < kFarMasks; q++) {
              while (rest[q] != 0ull && !full) {
                const int bit = __ffsll((long long)rest[q]) - 1;
                const int bx = 4 * (int)(spos[q] & 0x1fffffull) + (bit & 3), by = 4 * (int)((spos[q] >> 21) & 0x1fffffull) + ((bit >> 2) & 3), bz = 4 * (int)(spos[q] >> 42) + (bit >> 4);
                bool want = max(max(abs(bx - c[0]), abs(by - c[1])), abs(bz - c[2])) > kFarBlockShells;  // (else: phase A scanned it)
                if (want) want = box2(bx, by, bz) <= bound;
                if (want) {
                  const int slot = atomicAdd(&L.count, 1);
                  if (slot >= kFarList) {  // the list is full: this block waits for the next round
                    full = true;
                    break;
                  }
                  L.blk[slot] = (bz * dim[1] + by) * dim[0] + bx;
                }
                rest[q] &= rest[q] - 1ull;
              }
            }
          }
          wave_sync();
          const int nb = done ? 0 : min(L.count, kFarList);
          wave_sync();
          // (Scanning an unbounded group's nearest blocks first -- eight at a time until it holds k candidates, the rest against that bound -- cuts an outlier's candidates
          // from 1500 to 350 per lane and not its time: the 160-260 us of such a query are the ~35 dependent mask trips of five empty shells, not the surface behind them.
          // Measured and removed: profiles/r05_c5_summary.txt item 7.)
          far_process(nb, [&](int j) { return (size_t)L.blk[j]; }, [](int) { return true; });
        }
        const bool ok = settled_within((double)R * S + sface, !done);
        if (!done && (ok || R >= rs_max)) done = true;
        if (__builtin_amdgcn_ballot_w64(!done && fresh > 0) != 0ull) {  // (a shell that brought nothing leaves the bound as it is: no merge)
          have = merge();
          bound = fmin(bound, kth);
          fresh = 0;
        }
      }
    }
    // ---- the k smallest of the group's lists, ascending (ties: smaller index) ----
    have = merge();
    if (active && sub == 0) {
      float* out = (!NORMALS || covs) ? covs + 9 * (size_t)i : nullptr;
      float* nout = NORMALS ? normals + 3 * (size_t)i : nullptr;
      if (have < k) {
        atomicAdd(num_short, 1);
        store_identity<NORMALS>(self.x, out, nout);
      } else {
        TopK<KMAX, false> fin;
        fin.init(k, kInf);
#pragma unroll
        for (int r = 0; r < KMAX; r++) fin.idx[r] = fin_i[r];
        covariance_from_neighbours<KMAX, false, NORMALS>(fin, points, k, out, nout, qx, qy, qz);
      }
    }
  }
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

#include "gp_covariance_rows.hpp"  // the row-tiled pass (GP_TUNE_KNN_STRUCTURE = 3): covariance_rows_kernel, covariance_settle_kernel

extern "C" {

namespace gp {  // (opened inside extern "C", as it always was: the two probe kernels keep their unmangled names)
// ---- the side stream of gp_estimate_covariances: a hardware queue that does NOT share a dispatch pipe with the caller's ----
// Two kernels on two HIP streams overlap only when their hardware queues sit on different pipes of the command processor: a pipe dispatches ONE grid at a time, and a
// grid with more workgroups than the device holds keeps its pipe until its last workgroup has been placed.  Measured (profiles/r05_c5_queue_pipes.txt): with the
// caller on queue 1 and the side stream on queue 3 the second covariance launch starts 8 us after the first; on queue 5 (the same process after bench.py's C4 phase had
// taken queues 2-4) it starts when the first launch's last workgroup is placed, 100 / 160 us later on the two 1 M-point clouds -- 0.07 ms per call.  HIP does not say
// which queue a stream gets, so the library asks the device: up to four low-priority streams are created (each gets a queue of its own from the runtime's pool for that
// priority), and the candidates are probed ONCE per host thread and device, beside the first caller stream that thread brings -- a grid of 6144 workgroups that holds two
// LDS-bound workgroups per CU for ~5 us each on the caller's stream, and one wave on the candidate that reports how long after the grid's first workgroup it got to run
// (~1 us on another pipe, the grid's whole dispatch on the same one).  The candidate with the shortest delay serves the thread's calls on that device from then on
// (~0.4 ms once).  Round 5 probed per caller stream (a 16-entry table keyed on the raw handle): an application that cycles streams re-paid 0.4 ms per new handle to save
// 0.07 ms per call, and a recycled handle inherited a stale choice -- a later caller stream on another pipe now simply keeps the first choice (correct either
// way: the choice only decides whether the two launches overlap).  gp_trim_device_cache() releases the thread's candidate streams, events and probe words.
__global__ void __launch_bounds__(256) pipe_probe_hog_kernel(unsigned long long* __restrict__ words, int ticks) {
  __shared__ float pad[12 * 1024];  // 48 KB: three workgroups per CU (160 KB of LDS), the wave slots stay free for the probe's wave
  pad[threadIdx.x * 48] = (float)threadIdx.x;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  if (blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(words, t0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  while (__builtin_amdgcn_s_memrealtime() - t0 < (unsigned long long)ticks) __builtin_amdgcn_s_sleep(8);
  if (pad[(threadIdx.x * 48 + 7) % (12 * 1024)] < -1.0f) words[2] = 1;  // (keeps the array)
}
__global__ void __launch_bounds__(64) pipe_probe_stamp_kernel(unsigned long long* __restrict__ words) {
  if (threadIdx.x != 0) return;
  const unsigned long long t0 = __builtin_amdgcn_s_memrealtime();
  unsigned long long seen = 0;
  while ((seen = __hip_atomic_load(words, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT)) == 0 && __builtin_amdgcn_s_memrealtime() - t0 < 200000ull) __builtin_amdgcn_s_sleep(4);  // (<= 2 ms)
  words[1] = __builtin_amdgcn_s_memrealtime();
}

struct SideStreamHandles {
  hipStream_t stream = nullptr;
  hipEvent_t fork = nullptr, join = nullptr;
};
struct SideStream : SideStreamHandles {
  static constexpr int kCandidates = 4;
  struct PerDevice {
    SideStreamHandles cand[kCandidates];
    int num = 0;
    unsigned long long* words = nullptr;  // device: [0] first workgroup of the hog started, [1] the probe's wave ran, [2] unused
    struct Choice {
      hipStream_t caller;
      int index;
      float delay_us[kCandidates];
    } chosen{nullptr, 0, {-1.f, -1.f, -1.f, -1.f}};
    bool probed = false;
    bool created = false;
  };
  // releases what this thread holds for the current device (gp_trim_device_cache): the next covariance call creates and probes again
  static void release() {
    PerDevice* c = device_state();
    if (!c || !c->created) return;
    for (int i = 0; i < c->num; i++) {
      if (c->cand[i].stream) (void)hipStreamSynchronize(c->cand[i].stream), (void)hipStreamDestroy(c->cand[i].stream);
      if (c->cand[i].fork) (void)hipEventDestroy(c->cand[i].fork);
      if (c->cand[i].join) (void)hipEventDestroy(c->cand[i].join);
    }
    if (c->words) (void)hipFree(c->words);
    (void)hipGetLastError();
    *c = PerDevice{};
  }
  static PerDevice* device_state() {
    static thread_local PerDevice cache[16];
    int d = 0;
    if (hipGetDevice(&d) != hipSuccess || d < 0 || d >= 16) return nullptr;
    return &cache[d];
  }
  static void create(PerDevice& c) {
    c.created = true;
    // the LOWEST priority the device offers: what runs on the side stream fills the slots the caller's stream leaves free, it does not compete for them
    int least = 0, greatest = 0;
    if (hipDeviceGetStreamPriorityRange(&least, &greatest) != hipSuccess) least = 0, (void)hipGetLastError();
    for (int i = 0; i < kCandidates; i++) {
      SideStreamHandles n;
      if (hipStreamCreateWithPriority(&n.stream, hipStreamNonBlocking, least) != hipSuccess || hipEventCreateWithFlags(&n.fork, hipEventDisableTiming) != hipSuccess ||
          hipEventCreateWithFlags(&n.join, hipEventDisableTiming) != hipSuccess) {
        (void)hipGetLastError();
        break;
      }
      c.cand[c.num++] = n;
    }
    if (c.num > 1 && hipMalloc(&c.words, 4 * sizeof(unsigned long long)) != hipSuccess) (void)hipGetLastError(), c.words = nullptr;
  }
  // delay (us) between the first workgroup of a pipe-filling grid on `caller` and a wave on the candidate; < 0: the probe did not run
  static float probe(PerDevice& c, hipStream_t caller, const SideStreamHandles& n) {
    unsigned long long h[2] = {0, 0};
    if (hipMemsetAsync(c.words, 0, 4 * sizeof(unsigned long long), caller) != hipSuccess || hipEventRecord(n.fork, caller) != hipSuccess ||
        hipStreamWaitEvent(n.stream, n.fork, 0) != hipSuccess) {
      (void)hipGetLastError();
      return -1.f;
    }
    hipLaunchKernelGGL(pipe_probe_hog_kernel, dim3(6144), dim3(256), 0, caller, c.words, 500);
    hipLaunchKernelGGL(pipe_probe_stamp_kernel, dim3(1), dim3(64), 0, n.stream, c.words);
    if (hipEventRecord(n.join, n.stream) != hipSuccess || hipStreamWaitEvent(caller, n.join, 0) != hipSuccess) (void)hipStreamSynchronize(n.stream);
    if (hipStreamSynchronize(caller) != hipSuccess || hipMemcpy(h, c.words, sizeof(h), hipMemcpyDeviceToHost) != hipSuccess || h[0] == 0 || h[1] == 0) {
      (void)hipGetLastError();
      return -1.f;
    }
    return h[1] >= h[0] ? (float)(h[1] - h[0]) / 100.f : 0.f;  // 100 MHz
  }
  static int get(hipStream_t caller, SideStream* out, const PerDevice::Choice** report = nullptr) {
    PerDevice* c = device_state();
    if (!c) return fail(GP_ERROR_HIP, "SideStream: no current device");
    if (!c->created) create(*c);
    if (c->num == 0) return fail(GP_ERROR_HIP, "SideStream: cannot create the side stream");
    if (c->probed) {
      static_cast<SideStreamHandles&>(*out) = c->cand[c->chosen.index];
      if (report) *report = &c->chosen;
      return GP_OK;
    }
    PerDevice::Choice pick{caller, 0, {-1.f, -1.f, -1.f, -1.f}};
    c->probed = true;  // (once per thread and device, whatever comes of it)
    if (c->words) {
      for (int i = 0; i < c->num; i++) {
        // (two probes, the smaller delay: a first launch on a new queue pays for the queue)
        const float a = probe(*c, caller, c->cand[i]), b = probe(*c, caller, c->cand[i]);
        pick.delay_us[i] = a < 0.f ? b : b < 0.f ? a : std::min(a, b);
        if (pick.delay_us[i] >= 0.f && (pick.delay_us[pick.index] < 0.f || pick.delay_us[i] < pick.delay_us[pick.index] - 2.f)) pick.index = i;  // (ties within 2 us: the earlier one)
      }
    }
    c->chosen = pick;
    if (report) *report = &c->chosen;
    static_cast<SideStreamHandles&>(*out) = c->cand[pick.index];
    return GP_OK;
  }
};
extern "C++" void release_side_streams() { SideStream::release(); }  // (gp_trim_device_cache, gp_runtime.hip; declared in gp_host.hpp)
}  // namespace gp

// measurement / tests: the side stream gp_estimate_covariances uses beside `caller` on the current device -- the delays (us) the pipe probe measured for the (up to four)
// candidate streams (< 0: not probed) and the index of the one in use
int gp_debug_side_stream_probe(gp_stream_t caller, float delays_us[4], int* chosen) {
  gp::SideStream side;
  const gp::SideStream::PerDevice::Choice* report = nullptr;
  GP_TRY(gp::SideStream::get((hipStream_t)caller, &side, &report));
  for (int i = 0; i < 4; i++)
    if (delays_us) delays_us[i] = report ? report->delay_us[i] : -1.f;
  if (chosen) *chosen = report ? report->index : 0;
  return GP_OK;
}

int gp_estimate_covariances(const float* points_dev, int n, int k, double cell_size, float* covs_dev, int* num_short, gp_stream_t stream) {
  return gp_estimate_covariances_ex(points_dev, n, k, cell_size, covs_dev, num_short, 0, nullptr, stream);
}

// One search, the covariances (NORMALS = false: gp_estimate_covariances, the kernels as they always were) or the normals and / or the covariances (NORMALS = true:
// gp_estimate_normals_covariances; covs_dev may be null).  The flag is a template parameter of every kernel behind it: the covariance call keeps its registers.
extern "C++" template <bool NORMALS>
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
  const bool heavy_first = g->binned && g->structure != 6 && g->structure != 3 && !g->bin_levels.empty() && g->bin_levels[0]->bins.cell_of.ptr;
  // round 5: sparse neighbourhoods are handed to covariance_far_kernel (one wave per query); structure 7 = round 4's search (every query lane by lane) for the A/B
  const bool coop_far = heavy_first && g->structure == 0 && g->bin_levels.size() == 1 && k <= 10;
  int rc = GP_OK;
  if (rc == GP_OK) {
    if (!zeroed) (void)hipMemsetAsync(d_short.ptr, 0, zero_bytes, s);
    const gp::SearchView v = g->view();
    const int nq = g->binned ? g->num_binned : n;  // queries = the cell-sorted points; non-finite points are not among them
    if (nq < n) hipLaunchKernelGGL(gp::nonfinite_identity_kernel<NORMALS>, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, n, covs_dev, d_short.as<int>(), normals_dev);
    const dim3 grid((nq + 127) / 128), block(128);
    gp::DeviceArray todo;  // [nq] positions + the count behind them
    gp::DeviceArray scan_buf;  // RowScanOut: kept [kTileKeep][nq] | bound [nq] | safe [nq]
    const int* d_todo = nullptr;
    if (nq > 0 && g->binned && g->structure == 3 && k <= 10) {
      // tiled pass over the occupied cell rows of the finest level; what it cannot settle is listed for the per-lane pass
      rc = todo.alloc_async(sizeof(int) * ((size_t)nq + 1), s);
      if (rc == GP_OK) rc = scan_buf.alloc_async(sizeof(int) * (size_t)(gp::kTileKeep + 2) * nq, s);
      if (rc == GP_OK) {
        (void)hipMemsetAsync(todo.as<int>() + nq, 0, sizeof(int), s);
        const gp::RowScanOut scan{scan_buf.as<int>(), reinterpret_cast<float*>(scan_buf.as<int>() + (size_t)gp::kTileKeep * nq),
                                  reinterpret_cast<float*>(scan_buf.as<int>() + (size_t)(gp::kTileKeep + 1) * nq), nq};
        hipLaunchKernelGGL(gp::covariance_rows_kernel, dim3(16u * (unsigned)g->bin_levels[0]->bins.num_occ_blocks), dim3(gp::kRowThreads), 0, s, v.bins[0],
                           (const int*)g->bin_levels[0]->bins.occ_blocks.as<int>(), scan, 0);
        hipLaunchKernelGGL((gp::covariance_settle_kernel<10, NORMALS>), grid, block, 0, s, v.bins[0].sorted, scan, points_dev, k, covs_dev, todo.as<int>(), todo.as<int>() + nq,
                           normals_dev);
        d_todo = todo.as<int>();
      }
    }
    gp::DeviceArray heavy_before;
    if (nq > 0 && rc == GP_OK && heavy_first && !d_todo) {
      // heavy queries first (HeavyCellCount above): order[] = positions with own-cell population < k, then the rest; one scan over the cells + one scatter
      const gp::PointBins& bins = g->bin_levels[0]->bins;
      const int nc = bins.num_cells;
      rc = todo.alloc_async(sizeof(int) * ((size_t)nq + 2), s);
      if (rc == GP_OK) rc = heavy_before.alloc_async(sizeof(int) * (size_t)nc, s);
      if (rc == GP_OK) {
        int* d_heavy = todo.as<int>() + nq + 1;
        rc = gp::exclusive_scan_of(gp::HeavyCellCount{bins.cell_start.as<int>(), k}, heavy_before.as<int>(), nc, d_heavy, s,
                                   reinterpret_cast<unsigned long long*>(d_short.as<char>() + 256));
        if (rc == GP_OK) {
          hipLaunchKernelGGL(gp::heavy_first_order_kernel, dim3((nq + 255) / 256), dim3(256), 0, s, (const int*)bins.cell_start.as<int>(), (const unsigned*)bins.cell_of.as<unsigned>(),
                             (const int*)heavy_before.as<int>(), (const int*)d_heavy, k, nq, todo.as<int>());
          d_todo = todo.as<int>();
        }
      }
    }
    gp::DeviceArray far;  // positions (cell-sorted array) of the queries left to the cooperative kernel + their k-th distances so far; the count is word 1 of the zeroed block
    int *d_far = nullptr, *d_far_count = nullptr;
    float* d_far_bound = nullptr;
    if (nq > 0 && rc == GP_OK && coop_far) {
      rc = far.alloc_async((sizeof(int) + sizeof(float)) * (size_t)nq, s);
      if (rc == GP_OK) d_far = far.as<int>(), d_far_bound = reinterpret_cast<float*>(far.as<int>() + nq), d_far_count = d_short.as<int>() + 1;
    }
    if (nq > 0 && rc == GP_OK) {
      constexpr int cov_waves = 4;      // registers capped at 128 for four waves per SIMD (uncapped, three waves: 1.41 vs 1.28 ms, round 2)
      constexpr bool cov_full = true;   // k = 10: the straight-line insertion of full lists (profiles/r03_c5_straightline.txt)
      const int* d_count = d_todo ? d_todo + nq : nullptr;
      gp::SideStream side;
      if (d_far && k == 10 && gp::SideStream::get(s, &side) == GP_OK) {
        // Round 5: TWO launches of the same kernel on two streams.  The heavy part of the order (own-cell population < k: the only queries that can turn out sparse)
        // runs on `s` with the deferral, covariance_far_kernel behind it; the rest runs beside it on a side stream.  The far kernel is a few hundred waves bound by
        // the latency of its round trips (150-200 us for 0.15 % of the queries): behind ONE launch it would be added to the call, here it runs under the other
        // launch's waves.  Both cover the whole order with their grids and leave by the counts on the device (the split is not known to the host).
        const int* d_heavy = d_todo + nq + 1;
        bool forked = hipEventRecord(side.fork, s) == hipSuccess && hipStreamWaitEvent(side.stream, side.fork, 0) == hipSuccess;
        hipLaunchKernelGGL((gp::covariance_kernel<10, 4, true, NORMALS>), grid, block, 0, s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_heavy, d_far, d_far_count, d_far_bound,
                           (const int*)nullptr, normals_dev);
        hipLaunchKernelGGL((gp::covariance_kernel<10, 4, true, NORMALS>), grid, block, 0, forked ? side.stream : s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_count,
                           (int*)nullptr, (int*)nullptr, (float*)nullptr, d_heavy, normals_dev);
        const unsigned far_wgs = (unsigned)std::min<long long>(((long long)nq + 3) / 4, 8192);  // one wave = four queries per workgroup
        hipLaunchKernelGGL((gp::covariance_far_kernel<10, NORMALS>), dim3(far_wgs), dim3(64), 0, s, v.bins[0], points_dev, k, covs_dev, d_short.as<int>(), (const int*)d_far, (const float*)d_far_bound,
                           (const int*)d_far_count, normals_dev);
        if (forked && (hipEventRecord(side.join, side.stream) != hipSuccess || hipStreamWaitEvent(s, side.join, 0) != hipSuccess)) {
          (void)hipStreamSynchronize(side.stream);  // (the join could not be queued: wait for the side stream here, the call is synchronous anyway)
        }
      } else {
        if (k == 10 && cov_waves == 4 && cov_full)  // (capped at 96 registers for five waves per SIMD: 41 spilled, 1.08 vs 1.07 ms -- no gain)
          hipLaunchKernelGGL((gp::covariance_kernel<10, 4, true, NORMALS>), grid, block, 0, s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_count, d_far, d_far_count, d_far_bound,
                             (const int*)nullptr, normals_dev);
        else if (k <= 10 && cov_waves == 4)
          hipLaunchKernelGGL((gp::covariance_kernel<10, 4, false, NORMALS>), grid, block, 0, s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_count, d_far, d_far_count, d_far_bound,
                             (const int*)nullptr, normals_dev);
        else if (k <= 10)
          hipLaunchKernelGGL((gp::covariance_kernel<10, 1, false, NORMALS>), grid, block, 0, s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_count, d_far, d_far_count, d_far_bound,
                             (const int*)nullptr, normals_dev);
        else
          hipLaunchKernelGGL((gp::covariance_kernel<32, 1, false, NORMALS>), grid, block, 0, s, v, points_dev, nq, k, covs_dev, d_short.as<int>(), d_todo, d_count, (int*)nullptr, (int*)nullptr, (float*)nullptr,
                             (const int*)nullptr, normals_dev);
        if (d_far) {
          // a fixed grid (the count stays on the device): 4 waves per workgroup, 4 queries per wave, every group of 16 lanes takes queries w, w + groups, ... of the list
          const unsigned far_wgs = (unsigned)std::min<long long>(((long long)nq + 3) / 4, 8192);
          hipLaunchKernelGGL((gp::covariance_far_kernel<10, NORMALS>), dim3(far_wgs), dim3(64), 0, s, v.bins[0], points_dev, k, covs_dev, d_short.as<int>(), (const int*)d_far, (const float*)d_far_bound,
                             (const int*)d_far_count, normals_dev);
        }
      }
    }
    // the count of short queries comes back through a host-mapped word, behind a one-thread kernel whose flag the host polls (a D2H copy is a copy kernel + the
    // stream synchronisation's wake-up: ~10 us more)
    int h_short = 0;
    {
      gp::HostWords hw;
      int frc = gp::HostWords::get(&hw);
      if (frc == GP_OK) frc = hw.finish(s, d_short.as<int>(), 13);
      if (frc == GP_OK) {
        h_short = reinterpret_cast<volatile int*>(hw.host)[13];
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) frc = gp::hip_fail(e, "covariance_kernel", __FILE__, __LINE__);
      }
      if (frc != GP_OK && rc == GP_OK) rc = frc;
    }
    if (num_short) *num_short = h_short;
    if (h_short > 0) fprintf(stderr, "warning: fewer than k neighbors found for %d points\n", h_short);  // covariance_estimation.cpp:28
  }
  // the structure was built and searched on `s` only, and `s` has been synchronised: its arrays go back to the pool in stream order
  // (gp_point_grid_destroy has to assume searches on other streams and synchronises the device: 1.4 ms in a process with many streams)
  for (auto& lv : g->bin_levels) {
    for (gp::DeviceArray* a : {&lv->bins.blocks, &lv->bins.cell_start, &lv->bins.order, &lv->bins.cell_of, &lv->bins.cell_block, &lv->bins.occ_blocks, &lv->sorted, &lv->super})
      a->release_on(s);
  }
  delete g;
  return rc;
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
