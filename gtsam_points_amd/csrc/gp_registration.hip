// gp_registration.hip -- global registration on the device: RANSAC hypotheses and the weighted N-point alignment.  Device counterparts of
// registration/impl/ransac_impl.hpp:24-191 and registration/alignment.cpp:11-139; the contract of every entry point is in include/gtsam_points_hip.h.  The target's
// occupancy set is gp_occupancy.hip's (gp_occupancy_grid.hpp), the matching gp_feature_match.hip's, the closed forms and the tree sum gp_alignment.hpp's.  f64
// arithmetic on the f32 device points; the arithmetic a host restatement has to reproduce to the bit (the polygon error, H) is written without fused multiply-adds:
// contraction is off for the whole unit and fma() is called where one is wanted.
#pragma clang fp contract(off)

#include <cmath>
#include <cstring>

#include "gp_alignment.hpp"
#include "gp_feature_match.hpp"
#include "gp_occupancy_grid.hpp"

namespace gp {

// ---- the weighted N-point alignment ---------------------------------------------------------------------------------------------------------------------------------

// in one workgroup: two tree reductions in LDS (fixed order, no floating-point atomics): sum of weights and weighted means, then H
__global__ __launch_bounds__(kAlignThreads) void align_points_kernel(const double* __restrict__ target, const double* __restrict__ source, const double* __restrict__ weights, int n,
                                                                     int dof, double* __restrict__ pose_out) {
  __shared__ double lds[9 * kAlignThreads];
  double m[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kAlignThreads) add_weighted(m, weights[i], point_f64(target, i), point_f64(source, i));
  block_sum(lds, m, 7);
  const Means mean = weighted_means(m);
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int i = threadIdx.x; i < n; i += kAlignThreads) {
    const Vec3 t = sub3(point_f64(target, i), mean.t), s = sub3(point_f64(source, i), mean.s);
    add_outer(h, weights[i], t, s);
  }
  block_sum(lds, h, 9);
  if (threadIdx.x == 0) pose_from_H(h, mean.t, mean.s, dof, pose_out);
}

// ---- RANSAC -------------------------------------------------------------------------------------------------------------------------------------------------------

// one edge of the polygon pre-rejection (ransac_impl.hpp:81-83)
__device__ __forceinline__ double poly_edge_error(const Vec3& ta, const Vec3& tb, const Vec3& sa, const Vec3& sb) {
  const double dt = norm3(sub3(ta, tb)), ds = norm3(sub3(sa, sb));
  return fabs(dt - ds) / fmax(fmax(dt, ds), 1e-6);
}

struct RansacState {
  int stop;        // set behind the chunk whose scored hypotheses cross the early-stop rate
  int num_list;    // surviving hypotheses of the current chunk
  int best_inliers;
  int best_iteration;
  int num_scored;
  int pad_;
  double best_pose[16];
};

struct RansacArrays {
  int* status;
  int* source_indices;  // [H][3]
  int* target_indices;  // [H][3]
  double* poses;        // [H][16]
  int* inliers;
};

// one thread per iteration of the chunk [begin, begin + count): resets its rows, draws (or takes) the sample, tests the sampled feature rows
__global__ __launch_bounds__(256) void ransac_sample_kernel(RansacState* state, RansacArrays a, int begin, int count, int samples, int num_source, uint64_t seed,
                                                            const int* __restrict__ given, const float* __restrict__ source_features, int dim) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k == 0) state->num_list = 0;
  if (k >= count) return;
  const int it = begin + k;
  int idx[3] = {-1, -1, -1};
  int status = GP_RANSAC_SCORED;
  if (state->stop) {
    status = GP_RANSAC_SKIPPED;
  } else if (given) {
    for (int j = 0; j < samples; j++) idx[j] = given[3 * (size_t)it + j];
  } else {
    unsigned draw = 0;
    int redraws = 0;
    for (int j = 0; j < samples && status == GP_RANSAC_SCORED; j++) {
      for (;;) {
        const int c = (int)ransac_sample_index(seed, (unsigned)it, draw++, (unsigned)num_source);
        if ((j > 0 && c == idx[0]) || (j > 1 && c == idx[1])) {
          if (++redraws > GP_RANSAC_MAX_REDRAWS) {
            status = GP_RANSAC_SAMPLE_FAILED;
            break;
          }
          continue;
        }
        idx[j] = c;
        break;
      }
    }
    if (status != GP_RANSAC_SCORED) idx[0] = idx[1] = idx[2] = -1;
  }
  if (status == GP_RANSAC_SCORED) {
    for (int j = 0; j < samples; j++) {
      const float* f = source_features + (size_t)idx[j] * dim;
      bool zero = true;
      for (int c = 0; c < dim; c++) zero &= fabs((double)f[c]) <= 1e-3;
      if (zero) status = GP_RANSAC_INVALID_FEATURE;
    }
  }
  a.status[it] = status;
  for (int j = 0; j < 3; j++) {
    a.source_indices[3 * (size_t)it + j] = idx[j];
    a.target_indices[3 * (size_t)it + j] = -1;
  }
  for (int j = 0; j < 16; j++) a.poses[16 * (size_t)it + j] = 0.0;
  a.inliers[it] = -1;
}

// the rows the matching kernel searches: the sample of every iteration that is still alive, -1 otherwise
__global__ __launch_bounds__(256) void ransac_rows_kernel(const RansacState* state, RansacArrays a, int begin, int count, int* __restrict__ rows) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= 3 * count) return;
  const int it = begin + k / 3;
  rows[k] = (!state->stop && a.status[it] == GP_RANSAC_SCORED) ? a.source_indices[3 * (size_t)begin + k] : -1;
}

// one thread per iteration: polygon pre-rejection, alignment, taboo list; a survivor joins the chunk's list
__global__ __launch_bounds__(256) void ransac_hypothesis_kernel(RansacState* state, RansacArrays a, int begin, int count, int samples, const float* __restrict__ target, const float* __restrict__ source,
                                                                const int* __restrict__ matched, double poly_error_thresh, const double* __restrict__ taboo_inv, int num_taboo,
                                                                double taboo_rot, double taboo_trans, int* __restrict__ list) {
  const int k = blockIdx.x * 256 + threadIdx.x;
  if (k >= count || state->stop) return;
  const int it = begin + k;
  if (a.status[it] != GP_RANSAC_SCORED) return;
  const bool three = samples == 3;
  const int* si = a.source_indices + 3 * (size_t)it;
  const int t0i = max(matched[3 * k], 0), t1i = max(matched[3 * k + 1], 0), t2i = three ? max(matched[3 * k + 2], 0) : -1;  // (no match: target 0, ransac_impl.hpp:64)
  a.target_indices[3 * (size_t)it] = t0i, a.target_indices[3 * (size_t)it + 1] = t1i, a.target_indices[3 * (size_t)it + 2] = t2i;
  const Vec3 s0 = point_f64(source, si[0]), s1 = point_f64(source, si[1]), s2 = three ? point_f64(source, si[2]) : Vec3{0, 0, 0};
  const Vec3 t0 = point_f64(target, t0i), t1 = point_f64(target, t1i), t2 = three ? point_f64(target, t2i) : Vec3{0, 0, 0};
  double max_error = poly_edge_error(t0, t1, s0, s1);  // (two samples: both edges are this one)
  if (three) max_error = fmax(max_error, fmax(poly_edge_error(t1, t2, s1, s2), poly_edge_error(t2, t0, s2, s0)));
  if (max_error > poly_error_thresh) {
    a.status[it] = GP_RANSAC_POLY_REJECTED;
    return;
  }
  Vec3 mt, ms;
  if (three) {
    mt = {((t0.x + t1.x) + t2.x) / 3.0, ((t0.y + t1.y) + t2.y) / 3.0, ((t0.z + t1.z) + t2.z) / 3.0};
    ms = {((s0.x + s1.x) + s2.x) / 3.0, ((s0.y + s1.y) + s2.y) / 3.0, ((s0.z + s1.z) + s2.z) / 3.0};
  } else {
    mt = {(t0.x + t1.x) / 2.0, (t0.y + t1.y) / 2.0, (t0.z + t1.z) / 2.0};
    ms = {(s0.x + s1.x) / 2.0, (s0.y + s1.y) / 2.0, (s0.z + s1.z) / 2.0};
  }
  double h[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  add_outer(h, 1.0, sub3(t0, mt), sub3(s0, ms));
  add_outer(h, 1.0, sub3(t1, mt), sub3(s1, ms));
  if (three) add_outer(h, 1.0, sub3(t2, mt), sub3(s2, ms));
  double pose[16];
  pose_from_H(h, mt, ms, samples == 3 ? 6 : 4, pose);
  for (int j = 0; j < 16; j++) a.poses[16 * (size_t)it + j] = pose[j];
  for (int b = 0; b < num_taboo; b++) {  // delta = taboo^-1 * T (:150)
    const double* q = taboo_inv + 16 * b;
    double d[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) d[3 * r + c] = (q[r] * pose[4 * c] + q[4 + r] * pose[4 * c + 1]) + q[8 + r] * pose[4 * c + 2];
    const Vec3 dt{((q[0] * pose[12] + q[4] * pose[13]) + q[8] * pose[14]) + q[12], ((q[1] * pose[12] + q[5] * pose[13]) + q[9] * pose[14]) + q[13],
                  ((q[2] * pose[12] + q[6] * pose[13]) + q[10] * pose[14]) + q[14]};
    const Vec3 v{d[7] - d[5], d[2] - d[6], d[3] - d[1]};  // 2 sin(angle) axis
    const double angle = atan2(norm3(v), ((d[0] + d[4]) + d[8]) - 1.0);
    if (angle < taboo_rot && norm3(dt) < taboo_trans) {
      a.status[it] = GP_RANSAC_TABOO;
      return;
    }
  }
  a.inliers[it] = 0;
  list[atomicAdd(&state->num_list, 1)] = it;
}

// behind the chunk's scoring kernel, one workgroup: the chunk's best scored hypothesis (most inliers, lowest iteration) against the best so far, and the early stop.
// (Its tree is its own: an integer arg-max whose tie rule -- the lowest iteration -- is the comparison below, beside an integer sum and an or; gp_alignment.hpp's
// block_reduce combines doubles one by one.)
__global__ __launch_bounds__(256) void ransac_select_kernel(RansacState* state, RansacArrays a, int begin, int count, double stop_above) {
  __shared__ int s_inl[256], s_it[256], s_scored[256], s_stop[256];
  if (state->stop) return;
  int inl = -1, best_it = -1, scored = 0, stop = 0;
  for (int k = threadIdx.x; k < count; k += 256) {
    const int it = begin + k;
    if (a.status[it] != GP_RANSAC_SCORED) continue;
    const int c = a.inliers[it];
    scored++;
    stop |= (double)c > stop_above;
    if (c > inl) inl = c, best_it = it;  // (ascending iteration per thread: strict > keeps the lowest)
  }
  s_inl[threadIdx.x] = inl, s_it[threadIdx.x] = best_it, s_scored[threadIdx.x] = scored, s_stop[threadIdx.x] = stop;
  __syncthreads();
  for (int off = 128; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off) {
      const int oi = s_inl[threadIdx.x + off], ot = s_it[threadIdx.x + off];
      if (ot >= 0 && (s_it[threadIdx.x] < 0 || oi > s_inl[threadIdx.x] || (oi == s_inl[threadIdx.x] && ot < s_it[threadIdx.x]))) s_inl[threadIdx.x] = oi, s_it[threadIdx.x] = ot;
      s_scored[threadIdx.x] += s_scored[threadIdx.x + off];
      s_stop[threadIdx.x] |= s_stop[threadIdx.x + off];
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    state->num_scored += s_scored[0];
    if (s_it[0] >= 0 && s_inl[0] > state->best_inliers) {
      state->best_inliers = s_inl[0];
      state->best_iteration = s_it[0];
      for (int j = 0; j < 16; j++) state->best_pose[j] = a.poses[16 * (size_t)s_it[0] + j];
    }
    if (s_stop[0]) state->stop = 1;
  }
}

// ---- host: gp_ransac_estimate_pose in its stages ----------------------------------------------------------------------------------------------------------------------

static int check_ransac(const float* target_points, int num_target, const float* source_points, int num_source, const float* target_features, const float* source_features, int dim,
                        const gp_ransac_params* p, const gp_ransac_result* result) {
  if (!p || !result) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: params or result is NULL");
  if (p->dof != 6 && p->dof != 4) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: dof must be 6 or 4");
  if (num_source < (p->dof == 6 ? 3 : 2)) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: fewer source points than samples");
  if (num_target < 1) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: the target is empty");
  if (dim < 1 || dim > GP_FEATURE_MAX_DIM) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: dim must be 1 .. 128");
  if (p->num_taboo < 0 || p->num_taboo > GP_RANSAC_MAX_TABOO || (p->num_taboo > 0 && !p->taboo_poses))
    return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: at most 64 taboo poses");
  if (p->max_iterations < 1 || p->chunk_iterations < 1) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: max_iterations and chunk_iterations must be positive");
  if (!(p->inlier_voxel_resolution > 0.0) || !std::isfinite(p->inlier_voxel_resolution))
    return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: the resolution must be positive and finite");
  if (!target_points || !source_points || !target_features || !source_features) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_ransac_estimate_pose: NULL array");
  return GP_OK;
}

// what the stages hand on.  The grid comes first: it is destroyed last, and its destructor waits for the stream every array below was used on.
struct RansacRun {
  const float *target_points, *source_points, *target_features, *source_features;
  int num_target, num_source, dim;
  const gp_ransac_params* params;
  hipStream_t stream;
  int H, chunk;  // iterations in all and per chunk
  gp_occupancy_grid grid;
  RansacArrays a;  // the caller's arrays, or own[] in the same order
  DeviceArray own[5], state, rows, matched, dists, list, taboo;
  RansacState init;               // (the sources of the two queued uploads live as long as the call)
  std::vector<double> taboo_inv;
};

template <typename T>
static int caller_or_own(T* given, size_t count, DeviceArray& own, hipStream_t s, T** out) {
  if (!given) {
    GP_TRY(own.alloc_async(sizeof(T) * count, s));
    given = own.as<T>();
  }
  *out = given;
  return GP_OK;
}

// stage 1: the per-iteration arrays, each the caller's or the call's own; one chunk's scratch; the state as it is before the first chunk
static int ransac_arrays(RansacRun& r, const gp_ransac_hypotheses* given) {
  const gp_ransac_hypotheses g = given ? *given : gp_ransac_hypotheses{};  // (none given: five NULLs)
  const size_t H = (size_t)r.H, chunk = (size_t)r.chunk;
  GP_TRY(caller_or_own(g.status, H, r.own[0], r.stream, &r.a.status));
  GP_TRY(caller_or_own(g.source_indices, 3 * H, r.own[1], r.stream, &r.a.source_indices));
  GP_TRY(caller_or_own(g.target_indices, 3 * H, r.own[2], r.stream, &r.a.target_indices));
  GP_TRY(caller_or_own(g.poses, 16 * H, r.own[3], r.stream, &r.a.poses));
  GP_TRY(caller_or_own(g.inliers, H, r.own[4], r.stream, &r.a.inliers));
  GP_TRY(r.state.alloc_async(sizeof(RansacState), r.stream));
  GP_TRY(r.rows.alloc_async(sizeof(int) * 3 * chunk, r.stream));
  GP_TRY(r.matched.alloc_async(sizeof(int) * 3 * chunk, r.stream));
  GP_TRY(r.dists.alloc_async(sizeof(double) * 3 * chunk, r.stream));
  GP_TRY(r.list.alloc_async(sizeof(int) * chunk, r.stream));
  GP_TRY(r.taboo.alloc_async(sizeof(double) * 16 * (size_t)std::max(r.params->num_taboo, 1), r.stream));
  std::memset(&r.init, 0, sizeof(r.init));
  r.init.best_inliers = -1;
  r.init.best_iteration = -1;
  set_identity16(r.init.best_pose);
  GP_HIP(hipMemcpyAsync(r.state.ptr, &r.init, sizeof(r.init), hipMemcpyHostToDevice, r.stream));
  return GP_OK;
}

// stage 2: the inverses of the taboo poses, to the device
static int ransac_taboo_inverses(RansacRun& r) {
  const int num_taboo = r.params->num_taboo;
  r.taboo_inv.assign(16 * (size_t)std::max(num_taboo, 1), 0.0);
  for (int b = 0; b < num_taboo; b++) {  // Isometry3d::inverse(): R^T, -R^T t
    const double* T = r.params->taboo_poses + 16 * b;
    double* q = r.taboo_inv.data() + 16 * b;
    for (int i = 0; i < 3; i++)
      for (int c = 0; c < 3; c++) q[4 * c + i] = T[4 * i + c];
    for (int i = 0; i < 3; i++) q[12 + i] = -((q[i] * T[12] + q[4 + i] * T[13]) + q[8 + i] * T[14]);
    q[15] = 1.0;
  }
  if (num_taboo) GP_HIP(hipMemcpyAsync(r.taboo.ptr, r.taboo_inv.data(), sizeof(double) * 16 * num_taboo, hipMemcpyHostToDevice, r.stream));
  return GP_OK;
}

// stage 3: per chunk six launches in stream order -- sample, rows, match, hypothesis, score, select
static int ransac_chunks(RansacRun& r, const int* sample_indices) {
  const gp_ransac_params* p = r.params;
  const int samples = p->dof == 6 ? 3 : 2;
  RansacState* state = r.state.as<RansacState>();
  const double stop_above = (double)r.num_source * p->early_stop_inlier_rate;
  for (int begin = 0; begin < r.H; begin += r.chunk) {
    const int count = std::min(r.chunk, r.H - begin);
    hipLaunchKernelGGL(ransac_sample_kernel, dim3(blocks_of(count)), dim3(256), 0, r.stream, state, r.a, begin, count, samples, r.num_source, p->seed, sample_indices,
                       r.source_features, r.dim);
    hipLaunchKernelGGL(ransac_rows_kernel, dim3(blocks_of(3 * (size_t)count)), dim3(256), 0, r.stream, state, r.a, begin, count, r.rows.as<int>());
    GP_HIP(hipGetLastError());
    GP_TRY(launch_feature_nn(r.target_features, r.num_target, r.source_features, r.num_source, r.dim, r.rows.as<int>(), 3 * count, &state->stop, r.matched.as<int>(),
                             r.dists.as<double>(), r.stream));
    hipLaunchKernelGGL(ransac_hypothesis_kernel, dim3(blocks_of(count)), dim3(256), 0, r.stream, state, r.a, begin, count, samples, r.target_points, r.source_points,
                       r.matched.as<int>(), p->poly_error_thresh, r.taboo.as<double>(), p->num_taboo, p->taboo_thresh_rot, p->taboo_thresh_trans, r.list.as<int>());
    GP_HIP(hipGetLastError());
    GP_TRY(launch_overlap_batch(&r.grid, r.source_points, r.num_source, r.a.poses, r.list.as<int>(), &state->num_list, count, &state->stop, r.a.inliers, r.stream));
    hipLaunchKernelGGL(ransac_select_kernel, dim3(1), dim3(256), 0, r.stream, state, r.a, begin, count, stop_above);
    GP_HIP(hipGetLastError());
  }
  return GP_OK;
}

// stage 4: the one download, the call's one wait, the result
static int ransac_result(RansacRun& r, gp_ransac_result* result) {
  RansacState fin;
  GP_HIP(hipMemcpyAsync(&fin, r.state.ptr, sizeof(fin), hipMemcpyDeviceToHost, r.stream));
  GP_HIP(hipStreamSynchronize(r.stream));
  std::memcpy(result->T_target_source, fin.best_pose, sizeof(fin.best_pose));
  result->best_inliers = std::max(fin.best_inliers, 0);
  result->best_iteration = fin.best_iteration;
  result->num_scored = fin.num_scored;
  result->early_stopped = fin.stop;
  result->inlier_rate = (double)result->best_inliers / (double)r.num_target;
  return GP_OK;
}

}  // namespace gp

extern "C" {

void gp_ransac_params_default(gp_ransac_params* p) {
  if (!p) return;
  p->max_iterations = 5000;
  p->dof = 6;
  p->chunk_iterations = 1024;
  p->num_taboo = 0;
  p->early_stop_inlier_rate = 0.8;
  p->poly_error_thresh = 0.5;
  p->inlier_voxel_resolution = 1.0;
  p->taboo_thresh_rot = 0.5 * M_PI / 180.0;
  p->taboo_thresh_trans = 0.25;
  p->seed = 5489u;
  p->taboo_poses = nullptr;
}

unsigned gp_ransac_sample_index(uint64_t seed, unsigned iteration, unsigned draw, unsigned num_source) { return gp::ransac_sample_index(seed, iteration, draw, num_source); }

int gp_ransac_estimate_pose(const float* target_points_dev, int num_target, const float* source_points_dev, int num_source, const float* target_features_dev,
                            const float* source_features_dev, int dim, const gp_ransac_params* params, const int* sample_indices_dev, const gp_ransac_hypotheses* hypotheses,
                            gp_ransac_result* result, gp_stream_t stream) {
  using namespace gp;
  GP_TRY(check_ransac(target_points_dev, num_target, source_points_dev, num_source, target_features_dev, source_features_dev, dim, params, result));
  RansacRun r;
  r.target_points = target_points_dev, r.source_points = source_points_dev, r.target_features = target_features_dev, r.source_features = source_features_dev;
  r.num_target = num_target, r.num_source = num_source, r.dim = dim;
  r.params = params;
  r.stream = (hipStream_t)stream;
  r.H = params->max_iterations, r.chunk = std::min(params->chunk_iterations, r.H);
  // the target's occupancy set (:35-36), sized for the target at once and only queued: the download of the result is the call's one wait
  GP_TRY(grid_init(&r.grid, params->inlier_voxel_resolution, r.stream, num_target));
  GP_TRY(grid_insert(&r.grid, target_points_dev, num_target, nullptr, false));
  GP_TRY(ransac_arrays(r, hypotheses));
  GP_TRY(ransac_taboo_inverses(r));
  GP_TRY(ransac_chunks(r, sample_indices_dev));
  return ransac_result(r, result);
}

int gp_align_points(const double* target_points_dev, const double* source_points_dev, const double* weights_dev, int num_points, int dof, double* pose_out, gp_stream_t stream_) {
  if (dof != 6 && dof != 4) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_align_points: dof must be 6 or 4");
  if (num_points < 1 || !target_points_dev || !source_points_dev || !weights_dev || !pose_out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_align_points: bad arguments");
  hipStream_t stream = (hipStream_t)stream_;
  gp::DeviceArray pose_d;
  GP_TRY(pose_d.alloc_async(sizeof(double) * 16, stream));
  hipLaunchKernelGGL(gp::align_points_kernel, dim3(1), dim3(gp::kAlignThreads), 0, stream, target_points_dev, source_points_dev, weights_dev, num_points, dof, pose_d.as<double>());
  GP_HIP(hipGetLastError());
  GP_HIP(hipMemcpyAsync(pose_out, pose_d.ptr, sizeof(double) * 16, hipMemcpyDeviceToHost, stream));
  GP_HIP(hipStreamSynchronize(stream));
  return GP_OK;
}

}  // extern "C"
