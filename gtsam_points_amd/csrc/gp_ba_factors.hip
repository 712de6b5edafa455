// gp_ba_factors.hip -- PlaneEVMFactor / EdgeEVMFactor (factors/bundle_adjustment_factor_evm.hpp, balm_feature.hpp; Liu & Zhang, BALM, RA-L 2021) linearised on the
// device into gp_linearized6 records for the dense and sparse systems.  One factor is one feature (a plane or an edge) seen from K poses with N points; its error is
// an eigenvalue of the covariance of the transformed points q_i = T_pose(i) p_i (plane: lambda_0; edge: lambda_0 + lambda_1), f64 throughout.
//
// The reference forms a 3N x 3N point Hessian and multiplies it by a 3N x 6K Jacobian.  That Hessian is a block diagonal plus rank <= 3, so with
//   d_i = q_i - mean,  a_m(i) = d_i . u_m,  D_i^T v = (q_i x v ; v),  w_m(i) = a_m(i) u_k + a_k(i) u_m
//   s_a = sum_{i in a} D_i^T u_k,  g_{m,a} = sum D_i^T w_m(i),  B_a = sum (D_i^T u_k)(D_i^T u_k)^T,  r_a = sum a_k(i) D_i^T u_k
// the 6K x 6K factor of eigenvalue k is
//   G_ab = scale (2/N) [ delta_ab B_a - s_a s_b^T / N + sum_{m != k} g_{m,a} g_{m,b}^T / (N (lambda_k - lambda_m)) ],  g_a = -scale (2/N) r_a,  f = scale lambda_k.
// The edge factor is the sum over k = 0, 1 WITHOUT error_scale (EdgeEVMFactor::error / ::linearize ignore it); its (k = 0, m = 1) and (k = 1, m = 0) terms have the
// same w and opposite coefficients and are left out, only the m = 2 terms remain.  A repeated eigenvalue gives inf / NaN, as in the reference.
//
// Layout: the points of all features sorted by (feature, pose) -- a run of one feature's points on one pose is a SEGMENT.  Per segment 51 sums (a row): four
// 6-vectors V_0..V_3, the upper triangle of B (21) and r (6); per feature the weights that turn rows into blocks:
//   plane  V = (s, g_1, g_2, 0),                 coef = (-1/N, 1/(N(l0 - l1)), 1/(N(l0 - l2)), 0)
//   edge   V = (s^(0), s^(1), g_2^(0), g_2^(1)),  coef = (-1/N, -1/N, 1/(N(l0 - l2)), 1/(N(l1 - l2))),  B = B^(0) + B^(1),  r = r^(0) + r^(1)
//   G_ab = c [ delta_ab B_a + sum_j coef_j V_{j,a} V_{j,b}^T ],  c = scale 2/N.
// Launch 1 (ba_feature_kernel, one wave per feature): the mean (shifted by the feature's first point), the centred second moments, the eigenpairs (cyclic Jacobi,
// every lane the same operands: the same bits), then a lane per point fills a row in LDS and lanes 0-50 fold the rows into the segments' rows in point order.
// Launch 2 (ba_records_kernel, one workgroup per record): the contributions of a record -- listed by the host at create, in feature order -- are formed as outer
// products on the fly and summed in four interleaved parts that meet in a fixed order.  No atomics: two linearises at the same values are bit-identical.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "gp_host.hpp"

namespace gp {

constexpr int kBaRow = 51;   // V_0..V_3 at 0, 6, 12, 18; B at 24 (upper triangle, row by row); r at 45
constexpr int kBaFeat = 8;   // c, coef[4], f, N, 0
constexpr int kBaParts = 4;  // waves of a record's workgroup

struct BaView {
  const double* points;    // [num_points][3], sorted by (feature, pose)
  const int* point_seg;    // [num_points] the segment of a point
  const int* seg_pose;     // [S]
  const int* seg_points;   // [S + 1]
  const int* feat_points;  // [F + 1]
  const int* kinds;        // [F]
  const double* scales;    // [F]
};

struct BaContrib {
  int feature, seg_a, seg_b;
  int owner;  // the record takes this feature's f and point count (the unary record of the feature's lowest pose)
};

// q = T_pose(i) p_i (poses column-major 4x4)
__device__ __forceinline__ void ba_point(const BaView& v, const double* __restrict__ poses, int i, double* __restrict__ q) {
  const double* P = poses + 16 * (size_t)v.seg_pose[v.point_seg[i]];
  const double x = v.points[3 * (size_t)i], y = v.points[3 * (size_t)i + 1], z = v.points[3 * (size_t)i + 2];
#pragma unroll
  for (int r = 0; r < 3; r++) q[r] = P[r] * x + P[4 + r] * y + P[8 + r] * z + P[12 + r];
}

// one Jacobi rotation of the symmetric 3x3 in the (p, q) plane; r is the third index
__device__ __forceinline__ void ba_jacobi_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double* __restrict__ vp, double* __restrict__ vq) {
  if (apq == 0.0) return;
  const double theta = (aqq - app) / (2.0 * apq);
  const double t = copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
  const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
  app -= t * apq, aqq += t * apq, apq = 0.0;
  const double rp = arp, rq = arq;
  arp = c * rp - s * rq, arq = s * rp + c * rq;
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const double a = vp[k], b = vq[k];
    vp[k] = c * a - s * b, vq[k] = s * a + c * b;
  }
}

__device__ __forceinline__ void ba_order(double& la, double& lb, double* __restrict__ va, double* __restrict__ vb) {
  if (lb < la) {
    const double t = la;
    la = lb, lb = t;
#pragma unroll
    for (int k = 0; k < 3; k++) {
      const double x = va[k];
      va[k] = vb[k], vb[k] = x;
    }
  }
}

// eigenpairs of a symmetric 3x3 (a00 a01 a02 a11 a12 a22), ascending: cyclic Jacobi, a fixed number of sweeps (a converged pair is skipped)
__device__ __forceinline__ void ba_eig3(double a00, double a01, double a02, double a11, double a12, double a22, double* __restrict__ l, double* __restrict__ u0,
                                        double* __restrict__ u1, double* __restrict__ u2) {
  u0[0] = 1.0, u0[1] = 0.0, u0[2] = 0.0;
  u1[0] = 0.0, u1[1] = 1.0, u1[2] = 0.0;
  u2[0] = 0.0, u2[1] = 0.0, u2[2] = 1.0;
#pragma unroll 1
  for (int sweep = 0; sweep < 10; sweep++) {
    ba_jacobi_rotate(a00, a11, a01, a02, a12, u0, u1);
    ba_jacobi_rotate(a00, a22, a02, a01, a12, u0, u2);
    ba_jacobi_rotate(a11, a22, a12, a01, a02, u1, u2);
  }
  ba_order(a00, a11, u0, u1);
  ba_order(a11, a22, u1, u2);
  ba_order(a00, a11, u0, u1);
  l[0] = a00, l[1] = a11, l[2] = a22;
}

// D^T w = (q x w ; w) into out[0..5]
__device__ __forceinline__ void ba_dt(const double* __restrict__ q, double w0, double w1, double w2, double* __restrict__ out) {
  out[0] = q[1] * w2 - q[2] * w1, out[1] = q[2] * w0 - q[0] * w2, out[2] = q[0] * w1 - q[1] * w0;
  out[3] = w0, out[4] = w1, out[5] = w2;
}

// One wave per feature first + blockIdx.x.  LIN: the segments' rows into seg_table and the feature's weights into feat_table; else the feature's error alone.
template <bool LIN>
__global__ void __launch_bounds__(64) ba_feature_kernel(BaView v, const double* __restrict__ poses, int first, int count, double* __restrict__ seg_table,
                                                        double* __restrict__ feat_table, double* __restrict__ errors) {
  __shared__ double rows[LIN ? 64 * kBaRow : 1];
  __shared__ int seg_of[LIN ? 64 : 1];
  if ((int)blockIdx.x >= count) return;  // (the whole workgroup)
  const int f = first + blockIdx.x;
  const int lane = threadIdx.x;
  const int begin = v.feat_points[f], end = v.feat_points[f + 1];
  const double N = (double)(end - begin);
  // the mean, shifted by the feature's first point
  double c0[3], q[3];
  ba_point(v, poses, begin, c0);
  double s0 = 0.0, s1 = 0.0, s2 = 0.0;
  for (int i = begin + lane; i < end; i += 64) {
    ba_point(v, poses, i, q);
    s0 += q[0] - c0[0], s1 += q[1] - c0[1], s2 += q[2] - c0[2];
  }
  const double mean[3] = {c0[0] + wave_sum(s0) / N, c0[1] + wave_sum(s1) / N, c0[2] + wave_sum(s2) / N};
  // the centred second moments
  double m00 = 0.0, m01 = 0.0, m02 = 0.0, m11 = 0.0, m12 = 0.0, m22 = 0.0;
  for (int i = begin + lane; i < end; i += 64) {
    ba_point(v, poses, i, q);
    const double d0 = q[0] - mean[0], d1 = q[1] - mean[1], d2 = q[2] - mean[2];
    m00 += d0 * d0, m01 += d0 * d1, m02 += d0 * d2, m11 += d1 * d1, m12 += d1 * d2, m22 += d2 * d2;
  }
  double l[3], u0[3], u1[3], u2[3];
  ba_eig3(wave_sum(m00) / N, wave_sum(m01) / N, wave_sum(m02) / N, wave_sum(m11) / N, wave_sum(m12) / N, wave_sum(m22) / N, l, u0, u1, u2);
  const bool edge = v.kinds[f] == GP_BA_EDGE;
  const double scale = edge ? 1.0 : v.scales[f];  // (EdgeEVMFactor ignores error_scale)
  const double fval = edge ? l[0] + l[1] : scale * l[0];
  if (!LIN) {
    if (lane == 0) errors[f] = fval;
    return;
  }
  if (lane == 0) {
    double* ft = feat_table + kBaFeat * (size_t)f;
    ft[0] = scale * 2.0 / N;
    ft[1] = -1.0 / N;
    ft[2] = edge ? -1.0 / N : 1.0 / (N * (l[0] - l[1]));
    ft[3] = 1.0 / (N * (l[0] - l[2]));
    ft[4] = edge ? 1.0 / (N * (l[1] - l[2])) : 0.0;
    ft[5] = fval, ft[6] = N, ft[7] = 0.0;
  }
  // a lane per point fills a row; lanes 0-50 fold the rows of a segment, one entry each, in point order
  double acc = 0.0;
  for (int base = begin; base < end; base += 64) {
    const int i = base + lane;
    int sg = -1;
    if (i < end) {
      sg = v.point_seg[i];
      ba_point(v, poses, i, q);
      const double d0 = q[0] - mean[0], d1 = q[1] - mean[1], d2 = q[2] - mean[2];
      const double a0 = d0 * u0[0] + d1 * u0[1] + d2 * u0[2];
      const double a1 = d0 * u1[0] + d1 * u1[1] + d2 * u1[2];
      const double a2 = d0 * u2[0] + d1 * u2[1] + d2 * u2[2];
      double* row = rows + kBaRow * lane;
      double x0[6], x1[6], w[6];
      ba_dt(q, u0[0], u0[1], u0[2], x0);
      ba_dt(q, u1[0], u1[1], u1[2], x1);
#pragma unroll
      for (int k = 0; k < 6; k++) row[k] = x0[k];
      if (edge) {
#pragma unroll
        for (int k = 0; k < 6; k++) row[6 + k] = x1[k];
        ba_dt(q, a2 * u0[0] + a0 * u2[0], a2 * u0[1] + a0 * u2[1], a2 * u0[2] + a0 * u2[2], w);
#pragma unroll
        for (int k = 0; k < 6; k++) row[12 + k] = w[k];
        ba_dt(q, a2 * u1[0] + a1 * u2[0], a2 * u1[1] + a1 * u2[1], a2 * u1[2] + a1 * u2[2], w);
#pragma unroll
        for (int k = 0; k < 6; k++) row[18 + k] = w[k];
      } else {
        ba_dt(q, a1 * u0[0] + a0 * u1[0], a1 * u0[1] + a0 * u1[1], a1 * u0[2] + a0 * u1[2], w);
#pragma unroll
        for (int k = 0; k < 6; k++) row[6 + k] = w[k];
        ba_dt(q, a2 * u0[0] + a0 * u2[0], a2 * u0[1] + a0 * u2[1], a2 * u0[2] + a0 * u2[2], w);
#pragma unroll
        for (int k = 0; k < 6; k++) row[12 + k] = w[k], row[18 + k] = 0.0;
      }
      int at = 24;
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) row[at++] = edge ? x0[r] * x0[c] + x1[r] * x1[c] : x0[r] * x0[c];
#pragma unroll
      for (int k = 0; k < 6; k++) row[45 + k] = edge ? a0 * x0[k] + a1 * x1[k] : a0 * x0[k];
    }
    seg_of[lane] = sg;
    __syncthreads();
    if (lane < kBaRow) {
      const int n = min(64, end - base);
      for (int t = 0; t < n; t++) {
        acc += rows[kBaRow * t + lane];
        const int st = seg_of[t];
        if (base + t + 1 == v.seg_points[st + 1]) {  // the segment's last point
          seg_table[kBaRow * (size_t)st + lane] = acc;
          acc = 0.0;
        }
      }
    }
    __syncthreads();
  }
}

// One workgroup of kBaParts waves per record.  Entry e of a wave: e < 36 the block's (r, c) = (e % 6, e / 6); 36-41 the gradient side (unary); 42 the error;
// 43 the point count.  Wave p sums contributions p, p + kBaParts, ...; the parts meet as (0 + 1) + (2 + 3).
__global__ void __launch_bounds__(64 * kBaParts) ba_records_kernel(const int* __restrict__ rec_begin, const int* __restrict__ rec_pair, const BaContrib* __restrict__ contribs,
                                                                   const double* __restrict__ seg_table, const double* __restrict__ feat_table, int num_records,
                                                                   double* __restrict__ records) {
  __shared__ double part[kBaParts][64];
  __shared__ double total[64];
  const int rec = blockIdx.x;
  if (rec >= num_records) return;  // (the whole workgroup)
  const int e = threadIdx.x & 63, p = threadIdx.x >> 6;
  const bool pair = rec_pair[rec] != 0;
  const int begin = rec_begin[rec], end = rec_begin[rec + 1];
  double s = 0.0;
  if (e < 44) {
    const int r = e % 6, c = e / 6;
    const int lo = r < c ? r : c, hi = r < c ? c : r;
    const int sym = 24 + lo * 6 - lo * (lo - 1) / 2 + (hi - lo);  // (lo, hi) of the upper triangle stored row by row
    for (int k = begin + p; k < end; k += kBaParts) {
      const BaContrib q = contribs[k];
      const double* ft = feat_table + kBaFeat * (size_t)q.feature;
      const double* A = seg_table + kBaRow * (size_t)q.seg_a;
      const double* B = seg_table + kBaRow * (size_t)q.seg_b;
      if (e < 36) {
        double h = pair ? 0.0 : A[sym];
#pragma unroll
        for (int j = 0; j < 4; j++) h += ft[1 + j] * (A[6 * j + r] * B[6 * j + c]);
        s += ft[0] * h;
      } else if (e < 42) {
        if (!pair) s += ft[0] * A[45 + (e - 36)];
      } else if (q.owner) {
        s += e == 42 ? ft[5] : ft[6];
      }
    }
  }
  part[p][e] = s;
  __syncthreads();
  if (p == 0) total[e] = (part[0][e] + part[1][e]) + (part[2][e] + part[3][e]);
  __syncthreads();
  const int idx = threadIdx.x;
  if (idx < 122) {
    double val = 0.0;
    if (pair) {
      if (idx >= 74 && idx < 110) val = total[idx - 74];  // H_target_source: row = target, column = source
    } else {
      if (idx == 0) val = total[43];
      if (idx == 1) val = total[42];
      if (idx >= 38 && idx < 74) val = total[idx - 38];  // H_source
      if (idx >= 116) val = total[36 + (idx - 116)];     // b_source = -g
    }
    records[122 * (size_t)rec + idx] = val;
  }
}

static_assert(kBaParts == 4, "ba_records_kernel folds four parts");

}  // namespace gp

struct gp_ba_factors {
  hipStream_t stream = nullptr;
  int F = 0, N = 0, P = 0, S = 0, R = 0, U = 0;
  std::vector<int> feat_seg;            // [F + 1] the segments of a feature
  std::vector<int> seg_pose;            // [S]
  std::vector<int> rec_target, rec_source;  // [R] pose indices; target -1 = unary
  gp::DeviceArray d_points, d_point_seg, d_seg_pose, d_seg_points, d_feat_points, d_kinds, d_scales, d_rec_begin, d_rec_pair, d_contribs, d_seg_table, d_feat_table;
  gp::DeviceArray d_poses, d_out, d_tmp_begin, d_tmp_pair, d_tmp_contribs;
  // what create prepared on the host; uploaded (and dropped) by the first call that needs the device, so that create itself does no device work
  std::vector<double> h_points, h_scales;
  std::vector<int> h_point_seg, h_seg_points, h_feat_points, h_kinds, h_rec_begin, h_rec_pair;
  std::vector<gp::BaContrib> h_contribs;
  bool on_device = false;
  int tmp_feature = -1;  // whose record lists d_tmp_* hold (gp_ba_factors_feature_hessian)
  int ensure_device();
  gp::BaView view() const {
    return gp::BaView{d_points.as<double>(), d_point_seg.as<int>(), d_seg_pose.as<int>(), d_seg_points.as<int>(), d_feat_points.as<int>(), d_kinds.as<int>(), d_scales.as<double>()};
  }
};

int gp_ba_factors::ensure_device() {
  if (on_device) return GP_OK;
  GP_TRY(gp::upload(d_points, h_points));
  GP_TRY(gp::upload(d_point_seg, h_point_seg));
  GP_TRY(gp::upload(d_seg_pose, seg_pose));
  GP_TRY(gp::upload(d_seg_points, h_seg_points));
  GP_TRY(gp::upload(d_feat_points, h_feat_points));
  GP_TRY(gp::upload(d_kinds, h_kinds));
  GP_TRY(gp::upload(d_scales, h_scales));
  GP_TRY(gp::upload(d_rec_begin, h_rec_begin));
  GP_TRY(gp::upload(d_rec_pair, h_rec_pair));
  GP_TRY(gp::upload(d_contribs, h_contribs));
  GP_TRY(d_seg_table.alloc(sizeof(double) * gp::kBaRow * (size_t)S));
  GP_TRY(d_feat_table.alloc(sizeof(double) * gp::kBaFeat * (size_t)F));
  for (auto* v : {&h_point_seg, &h_seg_points, &h_feat_points, &h_kinds, &h_rec_begin, &h_rec_pair}) std::vector<int>().swap(*v);
  std::vector<double>().swap(h_points), std::vector<double>().swap(h_scales), std::vector<gp::BaContrib>().swap(h_contribs);
  on_device = true;
  return GP_OK;
}

namespace gp {

static int ba_launch_features(gp_ba_factors* b, const double* poses_dev, int first, int count, bool lin, double* errors_dev) {
  if (lin)
    hipLaunchKernelGGL(ba_feature_kernel<true>, dim3((unsigned)count), dim3(64), 0, b->stream, b->view(), poses_dev, first, count, b->d_seg_table.as<double>(),
                       b->d_feat_table.as<double>(), (double*)nullptr);
  else
    hipLaunchKernelGGL(ba_feature_kernel<false>, dim3((unsigned)count), dim3(64), 0, b->stream, b->view(), poses_dev, first, count, (double*)nullptr, (double*)nullptr, errors_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

static int ba_launch_records(gp_ba_factors* b, const int* rec_begin, const int* rec_pair, const BaContrib* contribs, int num_records, double* records_dev) {
  hipLaunchKernelGGL(ba_records_kernel, dim3((unsigned)num_records), dim3(64 * kBaParts), 0, b->stream, rec_begin, rec_pair, contribs, b->d_seg_table.as<double>(),
                     b->d_feat_table.as<double>(), num_records, records_dev);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

static int ba_poses_up(gp_ba_factors* b, const double* values_host) {
  GP_TRY(b->ensure_device());
  GP_TRY(b->d_poses.ensure(sizeof(double) * 16 * (size_t)b->P));
  GP_HIP(hipMemcpyAsync(b->d_poses.ptr, values_host, sizeof(double) * 16 * (size_t)b->P, hipMemcpyHostToDevice, b->stream));
  return GP_OK;
}

}  // namespace gp

extern "C" {

int gp_ba_factors_create(const int* kinds, const double* error_scales, const int* feature_offsets, const int* point_pose, const double* points, int num_features, int num_points,
                         int num_poses, gp_stream_t stream, gp_ba_factors_t** out) {
  const std::string api = "gp_ba_factors_create";
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": null out");
  *out = nullptr;
  if (!kinds || !error_scales || !feature_offsets || !point_pose || !points) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": null kinds, error_scales, feature_offsets, point_pose or points");
  if (num_features < 1 || num_points < 1 || num_poses < 1) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": num_features, num_points, num_poses >= 1");
  if (feature_offsets[0] != 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": feature_offsets[0] must be 0");
  for (int f = 0; f < num_features; f++) {
    const std::string at = api + ": feature " + std::to_string(f);
    if (kinds[f] != GP_BA_PLANE && kinds[f] != GP_BA_EDGE) return gp::fail(GP_ERROR_INVALID_ARGUMENT, at + ": unknown kind");
    if (feature_offsets[f + 1] < feature_offsets[f] || feature_offsets[f + 1] > num_points) return gp::fail(GP_ERROR_INVALID_ARGUMENT, at + ": feature_offsets are not sorted within [0, num_points]");
    if (feature_offsets[f + 1] - feature_offsets[f] < 3) return gp::fail(GP_ERROR_INVALID_ARGUMENT, at + ": fewer than 3 points");
    if (!std::isfinite(error_scales[f])) return gp::fail(GP_ERROR_INVALID_ARGUMENT, at + ": error_scale is not finite");
  }
  if (feature_offsets[num_features] != num_points) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": feature_offsets[num_features] must be num_points");
  for (int i = 0; i < num_points; i++)
    if (point_pose[i] < 0 || point_pose[i] >= num_poses) return gp::fail(GP_ERROR_INVALID_ARGUMENT, api + ": point " + std::to_string(i) + ": pose index outside [0, num_poses)");

  auto* b = new gp_ba_factors;
  b->stream = (hipStream_t)stream, b->F = num_features, b->N = num_points, b->P = num_poses;
  // the points of a feature sorted by pose (stable: a pose's points keep the caller's order), the runs of one pose = the segments
  std::vector<int> order(num_points), point_seg(num_points), seg_points, feat_points(feature_offsets, feature_offsets + num_features + 1);
  std::vector<double> sorted(3 * (size_t)num_points);
  b->feat_seg.assign(1, 0);
  for (int f = 0; f < num_features; f++) {
    const int lo = feature_offsets[f], hi = feature_offsets[f + 1];
    for (int i = lo; i < hi; i++) order[i] = i;
    std::stable_sort(order.begin() + lo, order.begin() + hi, [&](int x, int y) { return point_pose[x] < point_pose[y]; });
    for (int i = lo; i < hi; i++) {
      if (i == lo || point_pose[order[i]] != point_pose[order[i - 1]]) {
        b->seg_pose.push_back(point_pose[order[i]]);
        seg_points.push_back(i);
      }
      point_seg[i] = (int)b->seg_pose.size() - 1;
      std::memcpy(&sorted[3 * (size_t)i], points + 3 * (size_t)order[i], sizeof(double) * 3);
    }
    b->feat_seg.push_back((int)b->seg_pose.size());
  }
  seg_points.push_back(num_points);
  b->S = (int)b->seg_pose.size();
  // the records: a unary one per pose that a feature touches, in pose order, then one per co-observed pose pair a < b in (a, b) order; the contributions of a
  // record in feature order
  struct Item {
    int64_t key;
    gp::BaContrib c;
  };
  std::vector<Item> items;
  for (int f = 0; f < num_features; f++) {
    const int s0 = b->feat_seg[f], s1 = b->feat_seg[f + 1];
    for (int sa = s0; sa < s1; sa++) {
      items.push_back({(int64_t)b->seg_pose[sa], gp::BaContrib{f, sa, sa, sa == s0 ? 1 : 0}});
      for (int sb = sa + 1; sb < s1; sb++)
        items.push_back({((int64_t)b->seg_pose[sa] + 1) * (int64_t)num_poses + b->seg_pose[sb], gp::BaContrib{f, sa, sb, 0}});  // (every pair key >= num_poses: behind the unary ones)
    }
  }
  std::stable_sort(items.begin(), items.end(), [](const Item& x, const Item& y) { return x.key < y.key; });
  std::vector<int> rec_begin, rec_pair;
  std::vector<gp::BaContrib> contribs(items.size());
  for (size_t k = 0; k < items.size(); k++) {
    contribs[k] = items[k].c;
    if (k == 0 || items[k].key != items[k - 1].key) {
      const bool pair = items[k].key >= num_poses;
      rec_begin.push_back((int)k);
      rec_pair.push_back(pair ? 1 : 0);
      b->rec_target.push_back(pair ? (int)(items[k].key / num_poses) - 1 : -1);
      b->rec_source.push_back(pair ? (int)(items[k].key % num_poses) : (int)items[k].key);
      if (!pair) b->U++;
    }
  }
  rec_begin.push_back((int)items.size());
  b->R = (int)rec_pair.size();
  b->h_kinds.assign(kinds, kinds + num_features);
  b->h_scales.assign(error_scales, error_scales + num_features);
  b->h_points.swap(sorted), b->h_point_seg.swap(point_seg), b->h_seg_points.swap(seg_points), b->h_feat_points.swap(feat_points);
  b->h_rec_begin.swap(rec_begin), b->h_rec_pair.swap(rec_pair), b->h_contribs.swap(contribs);
  *out = b;
  return GP_OK;
}

int gp_ba_factors_destroy(gp_ba_factors_t* b) {
  if (!b) return GP_OK;
  if (b->on_device) (void)hipStreamSynchronize(b->stream);
  delete b;
  return GP_OK;
}

int gp_ba_factors_num_records(const gp_ba_factors_t* b) { return b ? b->R : 0; }

int gp_ba_factors_factor_slots(const gp_ba_factors_t* b, const int* slot_of_pose, int* out) {
  if (!b || !slot_of_pose || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_factor_slots: null");
  for (int r = 0; r < b->R; r++) {
    out[2 * r] = b->rec_target[r] < 0 ? -1 : slot_of_pose[b->rec_target[r]];
    out[2 * r + 1] = slot_of_pose[b->rec_source[r]];
  }
  return GP_OK;
}

int gp_ba_factors_issue_linearize_dev(gp_ba_factors_t* b, const double* poses_dev, gp_linearized6* records_dev) {
  if (!b || !poses_dev || !records_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_issue_linearize_dev: null");
  GP_TRY(b->ensure_device());
  GP_TRY(gp::ba_launch_features(b, poses_dev, 0, b->F, true, nullptr));
  return gp::ba_launch_records(b, b->d_rec_begin.as<int>(), b->d_rec_pair.as<int>(), b->d_contribs.as<gp::BaContrib>(), b->R, reinterpret_cast<double*>(records_dev));
}

int gp_ba_factors_linearize(gp_ba_factors_t* b, const double* values_host, gp_linearized6* records_host) {
  if (!b || !values_host || !records_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_linearize: null");
  const size_t bytes = sizeof(gp_linearized6) * (size_t)b->R;
  GP_TRY(gp::ba_poses_up(b, values_host));
  GP_TRY(b->d_out.ensure(bytes));
  GP_TRY(gp_ba_factors_issue_linearize_dev(b, b->d_poses.as<double>(), b->d_out.as<gp_linearized6>()));
  GP_HIP(hipMemcpyAsync(records_host, b->d_out.ptr, bytes, hipMemcpyDeviceToHost, b->stream));
  GP_HIP(hipStreamSynchronize(b->stream));
  return GP_OK;
}

int gp_ba_factors_compute_errors(gp_ba_factors_t* b, const double* values_host, double* errors_host) {
  if (!b || !values_host || !errors_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_compute_errors: null");
  const size_t bytes = sizeof(double) * (size_t)b->F;
  GP_TRY(gp::ba_poses_up(b, values_host));
  GP_TRY(b->d_out.ensure(bytes));
  GP_TRY(gp::ba_launch_features(b, b->d_poses.as<double>(), 0, b->F, false, b->d_out.as<double>()));
  GP_HIP(hipMemcpyAsync(errors_host, b->d_out.ptr, bytes, hipMemcpyDeviceToHost, b->stream));
  GP_HIP(hipStreamSynchronize(b->stream));
  return GP_OK;
}

int gp_ba_factors_feature_num_poses(const gp_ba_factors_t* b, int feature) {
  if (!b || feature < 0 || feature >= b->F) return 0;
  return b->feat_seg[feature + 1] - b->feat_seg[feature];
}

// the feature's own K + K (K - 1) / 2 records through the same two kernels, then copied (no arithmetic) into the dense factor
int gp_ba_factors_feature_hessian(gp_ba_factors_t* b, int feature, const double* values_host, double* G, double* g, double* f) {
  if (!b || !values_host || !G || !g || !f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_feature_hessian: null");
  if (feature < 0 || feature >= b->F) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ba_factors_feature_hessian: feature outside [0, num_features)");
  const int s0 = b->feat_seg[feature], K = b->feat_seg[feature + 1] - s0, R = K + K * (K - 1) / 2;
  std::vector<int> rec_begin(R + 1), rec_pair(R), ra(R), rb(R);
  std::vector<gp::BaContrib> contribs(R);
  int at = 0;
  for (int a = 0; a < K; a++, at++) contribs[at] = gp::BaContrib{feature, s0 + a, s0 + a, a == 0 ? 1 : 0}, rec_pair[at] = 0, ra[at] = a, rb[at] = a;
  for (int a = 0; a < K; a++)
    for (int c = a + 1; c < K; c++, at++) contribs[at] = gp::BaContrib{feature, s0 + a, s0 + c, 0}, rec_pair[at] = 1, ra[at] = a, rb[at] = c;
  for (int r = 0; r <= R; r++) rec_begin[r] = r;
  const size_t bytes = sizeof(gp_linearized6) * (size_t)R;
  GP_TRY(gp::ba_poses_up(b, values_host));
  // (the lists are kept between calls: a single-factor caller asks for the same feature at every linearise)
  GP_TRY(b->d_tmp_begin.ensure(sizeof(int) * (size_t)(R + 1)));
  GP_TRY(b->d_tmp_pair.ensure(sizeof(int) * (size_t)R));
  GP_TRY(b->d_tmp_contribs.ensure(sizeof(gp::BaContrib) * (size_t)R));
  if (b->tmp_feature != feature) {
    b->tmp_feature = -1;
    GP_HIP(hipMemcpy(b->d_tmp_begin.ptr, rec_begin.data(), sizeof(int) * (size_t)(R + 1), hipMemcpyHostToDevice));
    GP_HIP(hipMemcpy(b->d_tmp_pair.ptr, rec_pair.data(), sizeof(int) * (size_t)R, hipMemcpyHostToDevice));
    GP_HIP(hipMemcpy(b->d_tmp_contribs.ptr, contribs.data(), sizeof(gp::BaContrib) * (size_t)R, hipMemcpyHostToDevice));
    b->tmp_feature = feature;
  }
  GP_TRY(b->d_out.ensure(bytes));
  GP_TRY(gp::ba_launch_features(b, b->d_poses.as<double>(), feature, 1, true, nullptr));
  GP_TRY(gp::ba_launch_records(b, b->d_tmp_begin.as<int>(), b->d_tmp_pair.as<int>(), b->d_tmp_contribs.as<gp::BaContrib>(), R, b->d_out.as<double>()));
  std::vector<gp_linearized6> recs(R);
  GP_HIP(hipMemcpyAsync(recs.data(), b->d_out.ptr, bytes, hipMemcpyDeviceToHost, b->stream));
  GP_HIP(hipStreamSynchronize(b->stream));
  const size_t n = 6 * (size_t)K;
  *f = 0.0;
  for (int r = 0; r < R; r++) {
    const gp_linearized6& rec = recs[r];
    *f += rec.error;
    for (int c = 0; c < 6; c++)
      for (int q = 0; q < 6; q++) {
        if (ra[r] == rb[r]) {
          G[(6 * rb[r] + c) * n + 6 * ra[r] + q] = rec.H_source[c * 6 + q];
        } else {
          G[(6 * rb[r] + c) * n + 6 * ra[r] + q] = rec.H_target_source[c * 6 + q];
          G[(6 * ra[r] + q) * n + 6 * rb[r] + c] = rec.H_target_source[c * 6 + q];
        }
      }
    if (ra[r] == rb[r])
      for (int q = 0; q < 6; q++) g[6 * ra[r] + q] = -rec.b_source[q];
  }
  return GP_OK;
}

}  // extern "C"
