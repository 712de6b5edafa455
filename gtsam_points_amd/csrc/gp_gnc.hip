// gp_gnc.hip -- fast global registration on the device: reciprocal feature correspondences, the tuple test and the graduated non-convexity loop.  Device counterpart of
// registration/graduated_non_convexity.hpp and registration/impl/graduated_non_convexity_impl.hpp:27-198; the contract of every entry point is in
// include/gtsam_points_hip.h.  The matching is gp_feature_match.hip's feature_nn_kernel, the compaction gp_select.hpp's, the closed forms gp_alignment.hpp's.  f64
// arithmetic on the f32 device points; what a host restatement reproduces to the bit (errors, weights, mu) is written without fused multiply-adds.
#pragma clang fp contract(off)

#include <climits>
#include <cmath>
#include <cstring>

#include "gp_alignment.hpp"
#include "gp_feature_match.hpp"
#include "gp_select.hpp"

namespace gp {

// ---- correspondences (impl:27-84) -------------------------------------------------------------------------------------------------------------------------------------

// the K query rows of a cloud of n: the caller's, or the stratified rule of the header (K == n: every row)
__global__ __launch_bounds__(256) void gnc_query_rows_kernel(int n, int K, uint64_t seed, const int* __restrict__ given, int* __restrict__ rows) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= K) return;
  if (given) {
    rows[j] = given[j];
    return;
  }
  const long long lo = (long long)j * n / K, hi = ((long long)j + 1) * n / K;
  rows[j] = (int)lo + (int)ransac_sample_index(seed, (unsigned)j, 0u, (unsigned)(hi - lo));
}

// a query keeps its pair when it has a match and, with the reciprocal check, the match's own match is the query (:56-68)
__global__ __launch_bounds__(256) void gnc_keep_kernel(const int* __restrict__ rows, const int* __restrict__ forward, const int* __restrict__ back, int K, int* __restrict__ keep) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j < K) keep[j] = forward[j] >= 0 && (!back || back[j] == rows[j]);
}

// the kept pairs in order, (target, source): the query is the source row unless the roles were swapped (:75-80)
__global__ __launch_bounds__(256) void gnc_pairs_kernel(const int* __restrict__ selected, int count, const int* __restrict__ rows, const int* __restrict__ forward, int swapped,
                                                        int* __restrict__ pairs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  const int j = selected[i];
  pairs[2 * (size_t)i] = swapped ? rows[j] : forward[j];
  pairs[2 * (size_t)i + 1] = swapped ? forward[j] : rows[j];
}

// ---- tuple test (:91-131) -----------------------------------------------------------------------------------------------------------------------------------------------

// one thread per tuple: three draws, three edge ratios; the pairs of a valid tuple leave their target at their source's slot, the lowest target winning
__global__ __launch_bounds__(256) void gnc_tuple_kernel(const float* __restrict__ target, const float* __restrict__ source, const int* __restrict__ pairs, int count, int num_tuples,
                                                        uint64_t seed, double thresh, int* __restrict__ lowest_target) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= num_tuples) return;
  int ti[3], si[3];
  for (int k = 0; k < 3; k++) {
    const unsigned c = ransac_sample_index(seed, (unsigned)i, (unsigned)k, (unsigned)count);
    ti[k] = pairs[2 * (size_t)c], si[k] = pairs[2 * (size_t)c + 1];
  }
  const double upper = 1.0 / thresh;
  bool valid = true;
  for (int k = 0; k < 3; k++) {
    const int n = (k + 1) % 3;
    const double d1 = norm3(sub3(point_f64(target, ti[k]), point_f64(target, ti[n]))), d2 = norm3(sub3(point_f64(source, si[k]), point_f64(source, si[n])));
    const double ratio = d1 / d2;
    if (ratio < thresh || ratio > upper) valid = false;  // (NaN: neither)
  }
  if (!valid) return;
  for (int k = 0; k < 3; k++) atomicMin(&lowest_target[si[k]], ti[k]);
}

struct GncSourceKept {  // the flag of the tuple test's compaction: a source index some valid tuple holds
  const int* lowest_target;
  __device__ __forceinline__ int operator()(long long i) const { return lowest_target[i] != INT_MAX; }
};

__global__ __launch_bounds__(256) void gnc_tuple_pairs_kernel(const int* __restrict__ selected, int count, const int* __restrict__ lowest_target, int* __restrict__ pairs) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= count) return;
  pairs[2 * (size_t)i] = lowest_target[selected[i]];
  pairs[2 * (size_t)i + 1] = selected[i];
}

// ---- the loop (:133-198) ------------------------------------------------------------------------------------------------------------------------------------------------

// mu's start value: the diagonal of the bounding box of the points with three finite coordinates (:134-140); one workgroup, minima and maxima (any order gives the same)
__global__ __launch_bounds__(kAlignThreads) void gnc_diameter_kernel(const float* __restrict__ points, int n, double* __restrict__ mu0) {
  __shared__ double lds[6 * kAlignThreads];
  double box[6] = {INFINITY, INFINITY, INFINITY, -INFINITY, -INFINITY, -INFINITY};
  double *lo = box, *hi = box + 3;
  for (int i = threadIdx.x; i < n; i += kAlignThreads) {
    const Vec3 p = point_f64(points, i);
    if (!(fabs(p.x) < INFINITY && fabs(p.y) < INFINITY && fabs(p.z) < INFINITY)) continue;
    lo[0] = fmin(lo[0], p.x), lo[1] = fmin(lo[1], p.y), lo[2] = fmin(lo[2], p.z);
    hi[0] = fmax(hi[0], p.x), hi[1] = fmax(hi[1], p.y), hi[2] = fmax(hi[2], p.z);
  }
  block_reduce(lds, box, 6, [](int k, double a, double b) { return k < 3 ? fmin(a, b) : fmax(a, b); });  // one tree: three minima, three maxima
  if (threadIdx.x == 0) {
    const double dx = hi[0] - lo[0], dy = hi[1] - lo[1], dz = hi[2] - lo[2];
    *mu0 = lo[0] <= hi[0] ? sqrt((dx * dx + dy * dy) + dz * dz) : 0.0;
  }
}

// the pairs' points, contiguous: float[N][6] = target xyz, source xyz (the loop re-reads them from L2 in every alignment); an index outside its cloud is not read
__global__ __launch_bounds__(256) void gnc_gather_kernel(const float* __restrict__ target, int nt, const float* __restrict__ source, int ns, const int* __restrict__ pairs, int n,
                                                         float* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int t = pairs[2 * (size_t)i], s = pairs[2 * (size_t)i + 1];
  const bool ok = t >= 0 && t < nt && s >= 0 && s < ns;
  for (int c = 0; c < 3; c++) {
    out[6 * (size_t)i + c] = ok ? target[3 * (size_t)t + c] : __builtin_nanf("");
    out[6 * (size_t)i + 3 + c] = ok ? source[3 * (size_t)s + c] : __builtin_nanf("");
  }
}

struct GncPair {
  Vec3 t, s;
  double e, w;
};
// pair i at the pose (r row-major, tr): e = |t - T s|^2 (:161-164) and the weight (:165).  Both passes of an alignment call this: the same expression on the same operands.
__device__ __forceinline__ GncPair gnc_pair(const float* __restrict__ pairs6, int i, const double* r, const Vec3& tr, double mu, bool force_one) {
  const float* p = pairs6 + 6 * (size_t)i;
  GncPair g;
  g.t = {(double)p[0], (double)p[1], (double)p[2]};
  g.s = {(double)p[3], (double)p[4], (double)p[5]};
  const double dx = g.t.x - (((r[0] * g.s.x + r[1] * g.s.y) + r[2] * g.s.z) + tr.x);
  const double dy = g.t.y - (((r[3] * g.s.x + r[4] * g.s.y) + r[5] * g.s.z) + tr.y);
  const double dz = g.t.z - (((r[6] * g.s.x + r[7] * g.s.y) + r[8] * g.s.z) + tr.z);
  g.e = (dx * dx + dy * dy) + dz * dz;
  const double q = mu / (mu + g.e);
  g.w = force_one ? 1.0 : q * q;
  return g;
}

struct GncLoopOut {
  double pose[16];
  double inlier_rate;
  double final_mu;
  int num_alignments;
  int pad_;
};

// The whole loop in one workgroup: per alignment two strided passes over the pairs and two tree sums (weights, weighted means, errors, inliers; then H about the
// means), the pose by thread 0 into LDS.  mu's schedule runs here, by the reference's own sequence of divisions.  Any n >= 1.
__global__ __launch_bounds__(kAlignThreads) void gnc_loop_kernel(const float* __restrict__ pairs6, int n, const double* __restrict__ mu0, int dof, int max_iterations,
                                                                 int inner_iterations, double div_factor, double max_corr_dist, gp_gnc_trace trace, GncLoopOut* __restrict__ out) {
  __shared__ double lds[9 * kAlignThreads];
  __shared__ double s_pose[16];
  if (threadIdx.x < 16) s_pose[threadIdx.x] = threadIdx.x % 5 == 0 ? 1.0 : 0.0;
  __syncthreads();
  double mu = *mu0;
  const double inlier_thresh_sq = (2.0 * max_corr_dist) * (2.0 * max_corr_dist);
  double rate = 0.0;
  long long k = 0;
  for (int i = 0; i < max_iterations; i++) {
    for (int j = 0; j < inner_iterations; j++, k++) {
      const double r[9] = {s_pose[0], s_pose[4], s_pose[8], s_pose[1], s_pose[5], s_pose[9], s_pose[2], s_pose[6], s_pose[10]};
      const Vec3 tr{s_pose[12], s_pose[13], s_pose[14]};
      double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};  // sum w, w t, w s, e, inliers
      for (int c = threadIdx.x; c < n; c += kAlignThreads) {
        const GncPair g = gnc_pair(pairs6, c, r, tr, mu, i == 0 && c == 0);  // (:165: the correspondence index shadows the inner iteration)
        add_weighted(m, g.w, g.t, g.s);
        m[7] += g.e;
        m[8] += g.e < inlier_thresh_sq ? 1.0 : 0.0;
      }
      block_sum(lds, m, 9);
      const Means mean = weighted_means(m);
      double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int c = threadIdx.x; c < n; c += kAlignThreads) {
        const GncPair g = gnc_pair(pairs6, c, r, tr, mu, i == 0 && c == 0);
        add_outer(h, g.w, sub3(g.t, mean.t), sub3(g.s, mean.s));
      }
      block_sum(lds, h, 9);  // (its first barrier is behind every read of s_pose above)
      rate = m[8] / (double)n;
      if (threadIdx.x == 0) {
        pose_from_H(h, mean.t, mean.s, dof, s_pose);
        if (trace.mu) trace.mu[k] = mu;
        if (trace.sum_weights) trace.sum_weights[k] = m[0];
        if (trace.sum_errors) trace.sum_errors[k] = m[7];
        if (trace.num_inliers) trace.num_inliers[k] = (int)m[8];
      }
      __syncthreads();
      if (trace.poses && threadIdx.x < 16) trace.poses[16 * k + threadIdx.x] = s_pose[threadIdx.x];
    }
    mu /= div_factor;
    if (mu < max_corr_dist) break;
  }
  if (threadIdx.x < 16) out->pose[threadIdx.x] = s_pose[threadIdx.x];
  if (threadIdx.x == 0) {
    out->inlier_rate = rate;
    out->final_mu = mu;
    out->num_alignments = (int)k;
    out->pad_ = 0;
  }
}

// ---- host ---------------------------------------------------------------------------------------------------------------------------------------------------------------

static void identity_result(gp_gnc_result* r) {
  std::memset(r, 0, sizeof(*r));
  set_identity16(r->T_target_source);
}

static int check_clouds(const char* who, int num_target, int num_source, int dof) {
  if (dof != 6 && dof != 4) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": dof must be 6 or 4");
  if (num_target < 1 || num_source < 1) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": an empty cloud");
  return GP_OK;
}
static int check_matching(const char* who, const gp_gnc_params* p, int dim) {
  if (dim < 1 || dim > GP_FEATURE_MAX_DIM) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": dim must be 1 .. 128");
  if (p->max_init_samples < 1) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": max_init_samples must be positive");
  if (p->tuple_check && p->max_num_tuples < 1) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": max_num_tuples must be positive with tuple_check");
  return GP_OK;
}
static int check_loop(const char* who, const gp_gnc_params* p) {
  if (!(p->div_factor > 1.0)) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": div_factor must be above 1");
  if (!(p->max_corr_dist > 0.0)) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": max_corr_dist must be positive");
  if (p->max_iterations < 1 || p->inner_iterations < 1) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": max_iterations and inner_iterations must be positive");
  return GP_OK;
}

// stages 1 - 2 into pairs (int[K][2], K = *num_initial); two waits at most (the counts of the two compactions)
static int find_correspondences(const char* who, const float* tp, int nt, const float* sp, int ns, const float* tf, const float* sf, int dim, const gp_gnc_params* p, const int* given,
                                int num_given, int* pairs, int* count, int* num_initial, int* swapped_out, hipStream_t s) {
  const int swapped = ns < nt ? 0 : 1;
  const float *qf = swapped ? tf : sf, *of = swapped ? sf : tf;  // the query cloud's features, the other cloud's
  const int nq = swapped ? nt : ns, no = swapped ? ns : nt;
  const int K = given ? num_given : std::min(nq, p->max_init_samples);
  *swapped_out = swapped, *num_initial = K, *count = 0;
  if (K == 0) return GP_OK;
  DeviceArray rows, forward, back, dists, keep, selected;
  GP_TRY(rows.alloc_async(sizeof(int) * (size_t)K, s));
  GP_TRY(forward.alloc_async(sizeof(int) * (size_t)K, s));
  GP_TRY(back.alloc_async(sizeof(int) * (size_t)K, s));
  GP_TRY(dists.alloc_async(sizeof(double) * (size_t)K, s));
  GP_TRY(keep.alloc_async(sizeof(int) * (size_t)K, s));
  GP_TRY(selected.alloc_async(sizeof(int) * (size_t)K, s));
  hipLaunchKernelGGL(gnc_query_rows_kernel, dim3(blocks_of((size_t)K)), dim3(256), 0, s, nq, K, p->seed, given, rows.as<int>());
  GP_HIP(hipGetLastError());
  GP_TRY(launch_feature_nn(of, no, qf, nq, dim, rows.as<int>(), K, nullptr, forward.as<int>(), dists.as<double>(), s));
  if (p->reciprocal_check) GP_TRY(launch_feature_nn(qf, nq, of, no, dim, forward.as<int>(), K, nullptr, back.as<int>(), dists.as<double>(), s));
  hipLaunchKernelGGL(gnc_keep_kernel, dim3(blocks_of((size_t)K)), dim3(256), 0, s, (const int*)rows.as<int>(), (const int*)forward.as<int>(),
                     (const int*)(p->reciprocal_check ? back.as<int>() : nullptr), K, keep.as<int>());
  GP_HIP(hipGetLastError());
  GP_TRY(select_indices(ScanArrayInput{keep.as<int>(), 1}, K, selected.as<int>(), s, count, who));
  if (*count == 0) return GP_OK;
  hipLaunchKernelGGL(gnc_pairs_kernel, dim3(blocks_of((size_t)*count)), dim3(256), 0, s, (const int*)selected.as<int>(), *count, (const int*)rows.as<int>(),
                     (const int*)forward.as<int>(), swapped, pairs);
  GP_HIP(hipGetLastError());
  if (!p->tuple_check || (long long)*count <= 3LL * p->max_num_tuples) return GP_OK;
  DeviceArray lowest, kept;
  GP_TRY(lowest.alloc_async(sizeof(int) * (size_t)ns, s));
  GP_TRY(kept.alloc_async(sizeof(int) * (size_t)ns, s));
  GP_HIP(hipMemsetD32Async((hipDeviceptr_t)lowest.ptr, INT_MAX, (size_t)ns, s));
  hipLaunchKernelGGL(gnc_tuple_kernel, dim3(blocks_of((size_t)p->max_num_tuples)), dim3(256), 0, s, tp, sp, (const int*)pairs, *count, p->max_num_tuples, p->seed, p->tuple_thresh,
                     lowest.as<int>());
  GP_HIP(hipGetLastError());
  GP_TRY(select_indices(GncSourceKept{lowest.as<int>()}, ns, kept.as<int>(), s, count, who));  // (at most 3 max_num_tuples < the count before: they fit)
  if (*count == 0) return GP_OK;
  hipLaunchKernelGGL(gnc_tuple_pairs_kernel, dim3(blocks_of((size_t)*count)), dim3(256), 0, s, (const int*)kept.as<int>(), *count, (const int*)lowest.as<int>(), pairs);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

// stage 3: three launches (diameter, gather, loop) behind one wait
static int run_loop(const float* tp, int nt, const float* sp, int ns, const int* pairs, int n, const gp_gnc_params* p, const gp_gnc_trace* trace, gp_gnc_result* result, hipStream_t s) {
  result->num_correspondences = n;
  if (n == 0) return GP_OK;  // (the identity: set by the caller)
  DeviceArray pairs6, scalars;
  GP_TRY(pairs6.alloc_async(sizeof(float) * 6 * (size_t)n, s));
  GP_TRY(scalars.alloc_async(sizeof(double) * 2 + sizeof(GncLoopOut), s));
  double* mu0 = scalars.as<double>();
  GncLoopOut* out = reinterpret_cast<GncLoopOut*>(mu0 + 2);
  hipLaunchKernelGGL(gnc_diameter_kernel, dim3(1), dim3(kAlignThreads), 0, s, tp, nt, mu0);
  hipLaunchKernelGGL(gnc_gather_kernel, dim3(blocks_of((size_t)n)), dim3(256), 0, s, tp, nt, sp, ns, pairs, n, pairs6.as<float>());
  GP_HIP(hipGetLastError());
  gp_gnc_trace tr;
  std::memset(&tr, 0, sizeof(tr));
  if (trace) tr = *trace;
  hipLaunchKernelGGL(gnc_loop_kernel, dim3(1), dim3(kAlignThreads), 0, s, (const float*)pairs6.as<float>(), n, (const double*)mu0, p->dof, p->max_iterations, p->inner_iterations,
                     p->div_factor, p->max_corr_dist, tr, out);
  GP_HIP(hipGetLastError());
  GncLoopOut fin;
  GP_HIP(hipMemcpyAsync(&fin, out, sizeof(fin), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));
  std::memcpy(result->T_target_source, fin.pose, sizeof(fin.pose));
  result->inlier_rate = fin.inlier_rate;
  result->final_mu = fin.final_mu;
  result->num_alignments = fin.num_alignments;
  return GP_OK;
}

}  // namespace gp

extern "C" {

void gp_gnc_params_default(gp_gnc_params* p) {
  if (!p) return;
  p->max_init_samples = 5000;
  p->reciprocal_check = 1;
  p->tuple_check = 0;
  p->max_num_tuples = 1000;
  p->tuple_thresh = 0.9;
  p->div_factor = 1.4;
  p->max_corr_dist = 0.25;
  p->inner_iterations = 3;
  p->max_iterations = 64;
  p->dof = 6;
  p->reserved_ = 0;
  p->seed = 5489u;
}

int gp_feature_correspondences(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                               const float* source_features_dev, int dim, const gp_gnc_params* params, const int* query_indices_dev, int num_query_indices, int* pairs_out_dev,
                               int* num_pairs, int* num_initial, int* swapped, gp_stream_t stream) {
  using namespace gp;
  const char* who = "gp_feature_correspondences";
  if (!params || !num_pairs) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": params or num_pairs is NULL");
  if (num_target < 1 || num_source < 1) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": an empty cloud");
  GP_TRY(check_matching(who, params, dim));
  if (!target_features_dev || !source_features_dev || !pairs_out_dev || (params->tuple_check && (!target_points_dev || !source_points_dev)) ||
      (query_indices_dev && num_query_indices < 0))
    return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": NULL array");
  int initial = 0, swap = 0;
  GP_TRY(find_correspondences(who, target_points_dev, num_target, source_points_dev, num_source, target_features_dev, source_features_dev, dim, params, query_indices_dev,
                              num_query_indices, pairs_out_dev, num_pairs, &initial, &swap, (hipStream_t)stream));
  if (num_initial) *num_initial = initial;
  if (swapped) *swapped = swap;
  GP_HIP(hipStreamSynchronize((hipStream_t)stream));  // (the pairs are the caller's to read)
  return GP_OK;
}

int gp_gnc_align_correspondences(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const int* pairs_dev, int num_pairs,
                                 const gp_gnc_params* params, const gp_gnc_trace* trace, gp_gnc_result* result, gp_stream_t stream) {
  using namespace gp;
  const char* who = "gp_gnc_align_correspondences";
  if (!params || !result) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": params or result is NULL");
  GP_TRY(check_clouds(who, num_target, num_source, params->dof));
  GP_TRY(check_loop(who, params));
  if (num_pairs < 0 || !target_points_dev || !source_points_dev || (num_pairs > 0 && !pairs_dev)) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": NULL array");
  identity_result(result);
  return run_loop(target_points_dev, num_target, source_points_dev, num_source, pairs_dev, num_pairs, params, trace, result, (hipStream_t)stream);
}

int gp_gnc_estimate_pose(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                         const float* source_features_dev, int dim, const gp_gnc_params* params, const int* query_indices_dev, int num_query_indices, int* pairs_out_dev,
                         const gp_gnc_trace* trace, gp_gnc_result* result, gp_stream_t stream_) {
  using namespace gp;
  const char* who = "gp_gnc_estimate_pose";
  if (!params || !result) return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": params or result is NULL");
  GP_TRY(check_clouds(who, num_target, num_source, params->dof));
  GP_TRY(check_matching(who, params, dim));
  GP_TRY(check_loop(who, params));
  if (!target_points_dev || !source_points_dev || !target_features_dev || !source_features_dev || (query_indices_dev && num_query_indices < 0))
    return fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": NULL array");
  hipStream_t stream = (hipStream_t)stream_;
  identity_result(result);
  const int capacity = query_indices_dev ? num_query_indices : std::min(num_source < num_target ? num_source : num_target, params->max_init_samples);
  DeviceArray own;
  int* pairs = pairs_out_dev;
  if (!pairs) {
    GP_TRY(own.alloc_async(sizeof(int) * 2 * (size_t)std::max(capacity, 1), stream));
    pairs = own.as<int>();
  }
  int count = 0;
  GP_TRY(find_correspondences(who, target_points_dev, num_target, source_points_dev, num_source, target_features_dev, source_features_dev, dim, params, query_indices_dev,
                              num_query_indices, pairs, &count, &result->num_initial, &result->swapped, stream));
  return run_loop(target_points_dev, num_target, source_points_dev, num_source, pairs, count, params, trace, result, stream);
}

}  // extern "C"
