// gp_ct_factors.hip -- the continuous-time ICP and GICP factors: two pose variables (the sensor pose at the start and at the end of a sweep), every source point
// transformed by the pose interpolated at its own time stamp, a 12x12 Hessian over both poses.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/impl/integrated_ct_icp_factor_impl.hpp:41-55,92-308     time table, update_poses, correspondences, H/b, deskew   -> gp_ct_factor_* (kind 0)
//   factors/impl/integrated_ct_gicp_factor_impl.hpp:64-219          the same with the GICP term and the stored M             -> gp_ct_factor_* (kind 1)
//
// Four kinds of kernel, all of them here: the pose table (one lane per time bin: T(t), D0(t), D1(t), gp_pose3_ct.hpp), the 1-NN search with one pose per point on
// the search core of gp_knn_search.hpp, the tile kernel, the deskew.  The tile kernel never multiplies a point's Jacobian through D0 / D1: both are constant within
// a time bin, so a lane sums A = J^T M J (21) and g = J^T M r (6) in the local tangent of T(t) while its points stay in one bin and applies
// H_ab += D_a^T A D_b, b_a += D_a^T g when the bin changes -- time-sorted points in a tile share very few bins.  The 92 sums go into the two-key partial row of the
// VGICP factor's general path (gp_device.hpp ACCG: H_00 in the target slots, H_11 in the source slots, H_01 in the cross sums), whose finalize is a plain expansion.
#include "gp_corr_factors.hpp"
#include "gp_knn_search.hpp"
#include "gp_pose3_ct.hpp"

namespace gp {

// the poses ride in the kernel arguments, like CorrPoses
struct CtPoses {
  double pose0[16], pose1[16];
};

// update_poses (:202-248): one lane per table entry
__global__ void __launch_bounds__(64) ct_pose_table_kernel(const CtPoses poses, const double* __restrict__ times, int bins, int derivs, double* __restrict__ table) {
  const int b = blockIdx.x * 64 + threadIdx.x;
  if (b >= bins) return;
  ct_pose_entry(load_rigid(poses.pose0), load_rigid(poses.pose1), times[b], derivs != 0, table + (size_t)b * kCtPoseRow);
}

__device__ __forceinline__ Pose load_pose_row(const double* __restrict__ row /*3x4 row-major*/) {
  Pose p;
  p.r00 = row[0], p.r01 = row[1], p.r02 = row[2], p.tx = row[3];
  p.r10 = row[4], p.r11 = row[5], p.r12 = row[6], p.ty = row[7];
  p.r20 = row[8], p.r21 = row[9], p.r22 = row[10], p.tz = row[11];
  return p;
}

// update_correspondences (:251-288): nearest_correspond_kernel (gp_knn.hip) with the pose of the point's time bin -- corr[i] = the nearest target point of
// T(t_i) p_i with squared distance < max, or -1.  One query per lane and nothing else in the kernel.
struct CtSearchDesc {
  const float* points;
  const int* time_index;
  const double* table;  // [bins][kCtPoseRow]
  SearchView grid;
  int n;
  double max_sq_dist;
};

__global__ void __launch_bounds__(256) ct_nearest_kernel(CtSearchDesc f, int* __restrict__ corr) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= f.n) return;
  const Pose T = load_pose_row(f.table + (size_t)f.time_index[i] * kCtPoseRow);
  const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
  const double qx = T.r00 * px + T.r01 * py + T.r02 * pz + T.tx;
  const double qy = T.r10 * px + T.r11 * py + T.r12 * pz + T.ty;
  const double qz = T.r20 * px + T.r21 * py + T.r22 * pz + T.tz;
  TopK<1> top;
  top.init(1, f.max_sq_dist);
  knn_query_any<1>(f.grid, qx, qy, qz, 1, top);
  corr[i] = top.found ? top.idx[0] : -1;
}

// ---- the per-point terms: "given source point i, its target point j, the rows of its time bin in the linearisation and the evaluation pose table: in an error
// pass add to acc[ACC_COUNT] / acc[ACC_ERR]; in a linearise also to the local sums" ----
enum : int { LOC_A = 0, LOC_G = 21, LOC_SIZE = 27 };  // A = sum J^T M J, upper triangle row by row; g = sum J^T M r

struct CtDesc {
  const float* points;          // [n][3] source
  const float* covs;            // [n][9] source, GICP
  const int* time_index;        // [n]
  const float* target_points;   // [num_target][3]
  const float* target_normals;  // [num_target][3], ICP
  const float* target_covs;     // [num_target][9], GICP
};

// J = R [-[p]x, I], the derivative of T p in the local tangent of T (column j < 3: R (e_j x p))
__device__ __forceinline__ void ct_point_jacobian(const Pose& T, double px, double py, double pz, double (*J)[6]) {
  const double R[3][3] = {{T.r00, T.r01, T.r02}, {T.r10, T.r11, T.r12}, {T.r20, T.r21, T.r22}};
#pragma unroll
  for (int r = 0; r < 3; r++) {
    J[r][0] = R[r][2] * py - R[r][1] * pz;
    J[r][1] = R[r][0] * pz - R[r][2] * px;
    J[r][2] = R[r][1] * px - R[r][0] * py;
    J[r][3] = R[r][0];
    J[r][4] = R[r][1];
    J[r][5] = R[r][2];
  }
}

// (:141-182) e = n_B . (T p - x_B), the scalar residual; h = n_B^T J
struct CtIcpTerm {
  CtDesc f;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const double* __restrict__ row_lin, const double* __restrict__ row_eval, double* acc, double* loc) const {
    const Pose T = load_pose_row(row_eval);
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double nx = (double)f.target_normals[3 * j], ny = (double)f.target_normals[3 * j + 1], nz = (double)f.target_normals[3 * j + 2];
    const double rx = (T.r00 * px + T.r01 * py + T.r02 * pz + T.tx) - (double)f.target_points[3 * j];
    const double ry = (T.r10 * px + T.r11 * py + T.r12 * pz + T.ty) - (double)f.target_points[3 * j + 1];
    const double rz = (T.r20 * px + T.r21 * py + T.r22 * pz + T.tz) - (double)f.target_points[3 * j + 2];
    const double e = rx * nx + ry * ny + rz * nz;
    acc[ACC_COUNT] += 1.0;
    acc[ACC_ERR] += e * e;
    if constexpr (MODE != MODE_ERR) {
      double J[3][6], h[6];
      ct_point_jacobian(T, px, py, pz, J);
#pragma unroll
      for (int c = 0; c < 6; c++) h[c] = nx * J[0][c] + ny * J[1][c] + nz * J[2][c];
      int idx = LOC_A;
#pragma unroll
      for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = r; c < 6; c++) loc[idx++] += h[r] * h[c];
        loc[LOC_G + r] += h[r] * e;
      }
    }
  }
};

// (ct_gicp :107-151, :171-200) r = T p - x_B under M = (C_B + R C_A R^T)^-1 with R of the LINEARISATION pose table's entry, also in an error pass
struct CtGicpTerm {
  CtDesc f;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const double* __restrict__ row_lin, const double* __restrict__ row_eval, double* acc, double* loc) const {
    const Pose Tl = load_pose_row(row_lin);
    const Pose T = MODE == MODE_ERR ? load_pose_row(row_eval) : Tl;
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const float* cp = f.covs + 9 * (size_t)i;
    const float* cq = f.target_covs + 9 * j;
    // symmetric parts of both column-major 3x3 covariances, as the GICP term takes them
    const double ca[6] = {(double)cp[0], 0.5 * ((double)cp[3] + (double)cp[1]), 0.5 * ((double)cp[6] + (double)cp[2]),
                          (double)cp[4], 0.5 * ((double)cp[7] + (double)cp[5]), (double)cp[8]};
    const double cb[6] = {(double)cq[0], 0.5 * ((double)cq[3] + (double)cq[1]), 0.5 * ((double)cq[6] + (double)cq[2]),
                          (double)cq[4], 0.5 * ((double)cq[7] + (double)cq[5]), (double)cq[8]};
    double m[6];
    fused_mahalanobis(Tl, ca, cb, m);
    const double rx = (T.r00 * px + T.r01 * py + T.r02 * pz + T.tx) - (double)f.target_points[3 * j];
    const double ry = (T.r10 * px + T.r11 * py + T.r12 * pz + T.ty) - (double)f.target_points[3 * j + 1];
    const double rz = (T.r20 * px + T.r21 * py + T.r22 * pz + T.tz) - (double)f.target_points[3 * j + 2];
    const double w[3] = {m[0] * rx + m[1] * ry + m[2] * rz, m[1] * rx + m[3] * ry + m[4] * rz, m[2] * rx + m[4] * ry + m[5] * rz};
    acc[ACC_COUNT] += 1.0;
    acc[ACC_ERR] += rx * w[0] + ry * w[1] + rz * w[2];
    if constexpr (MODE != MODE_ERR) {
      double J[3][6], MJ[3][6];
      ct_point_jacobian(T, px, py, pz, J);
#pragma unroll
      for (int c = 0; c < 6; c++) {
        MJ[0][c] = m[0] * J[0][c] + m[1] * J[1][c] + m[2] * J[2][c];
        MJ[1][c] = m[1] * J[0][c] + m[3] * J[1][c] + m[4] * J[2][c];
        MJ[2][c] = m[2] * J[0][c] + m[4] * J[1][c] + m[5] * J[2][c];
      }
      int idx = LOC_A;
#pragma unroll
      for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = r; c < 6; c++) loc[idx++] += J[0][r] * MJ[0][c] + J[1][r] * MJ[1][c] + J[2][r] * MJ[2][c];
        loc[LOC_G + r] += J[0][r] * w[0] + J[1][r] * w[1] + J[2][r] * w[2];
      }
    }
  }
};

// where the entries of the two symmetric diagonal blocks live in the ACCG row (gp_device.hpp; expanded by vgicp_finalize_general_kernel), r <= c:
//   H_00 in the target slots: H_t = [[TL, -K^T], [-K, M]], so an entry of the off-diagonal 3x3 goes into K with its sign turned
//   H_11 in the source slots: [[HS_TL, HS_BL^T], [HS_BL, HS_BR]]
constexpr int ct_sym3(int a, int b) { return (a * (5 - a)) / 2 + b; }  // a <= b: 00 01 02 11 12 22
constexpr int ct_slot00(int r, int c) { return c < 3 ? ACC_TL + ct_sym3(r, c) : (r < 3 ? ACC_K + (c - 3) * 3 + r : ACC_M + ct_sym3(r - 3, c - 3)); }
constexpr int ct_slot11(int r, int c) { return c < 3 ? ACCG_HS_TL + ct_sym3(r, c) : (r < 3 ? ACCG_HS_BL + (c - 3) * 3 + r : ACCG_HS_BR + ct_sym3(r - 3, c - 3)); }
constexpr int ct_sym6(int a, int b) { return a <= b ? a * 6 - (a * (a - 1)) / 2 + (b - a) : b * 6 - (b * (b - 1)) / 2 + (a - b); }

// a lane leaves a time bin: H_ab += D_a^T A D_b, b_a += D_a^T g with the bin's D0 / D1 (row: its pose-table entry), then A = g = 0
__device__ __forceinline__ void ct_apply_bin(const double* __restrict__ row, double* loc, double* acc) {
  double D0[36], D1[36];
#pragma unroll
  for (int k = 0; k < 36; k++) {
    D0[k] = row[12 + k];
    D1[k] = row[48 + k];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double v0[6], v1[6];  // A D0[:, c], A D1[:, c]
#pragma unroll
    for (int k = 0; k < 6; k++) {
      double s0 = 0.0, s1 = 0.0;
#pragma unroll
      for (int m = 0; m < 6; m++) {
        s0 += loc[LOC_A + ct_sym6(k, m)] * D0[m * 6 + c];
        s1 += loc[LOC_A + ct_sym6(k, m)] * D1[m * 6 + c];
      }
      v0[k] = s0;
      v1[k] = s1;
    }
#pragma unroll
    for (int r = 0; r < 6; r++) {
      double h01 = 0.0;
#pragma unroll
      for (int k = 0; k < 6; k++) h01 += D0[k * 6 + r] * v1[k];
      acc[ACCG_HTS + 6 * r + c] += h01;
      if (r <= c) {
        double h00 = 0.0, h11 = 0.0;
#pragma unroll
        for (int k = 0; k < 6; k++) {
          h00 += D0[k * 6 + r] * v0[k];
          h11 += D1[k * 6 + r] * v1[k];
        }
        if (r < 3 && c >= 3)
          acc[ct_slot00(r, c)] -= h00;
        else
          acc[ct_slot00(r, c)] += h00;
        acc[ct_slot11(r, c)] += h11;
      }
    }
  }
#pragma unroll
  for (int r = 0; r < 6; r++) {
    double b0 = 0.0, b1 = 0.0;
#pragma unroll
    for (int k = 0; k < 6; k++) {
      b0 += D0[k * 6 + r] * loc[LOC_G + k];
      b1 += D1[k * 6 + r] * loc[LOC_G + k];
    }
    acc[(r < 3 ? ACC_QXMR : ACC_MR - 3) + r] += b0;
    acc[ACCG_BS + r] += b1;
  }
#pragma unroll
  for (int k = 0; k < LOC_SIZE; k++) loc[k] = 0.0;
}

// One workgroup per tile of `tile_points` points, lane t of 256 takes points t, t + 256, ... of its tile in that order and skips those without a target point
// within the cut-off: a fixed order, so two passes over the same correspondences are bit-identical.  MODE_LIN_GENERAL: the 92 sums; MODE_ERR: count and error.
template <int MODE, class TERM>
__global__ void __launch_bounds__(256) ct_tile_kernel(TERM f, const double* __restrict__ table_lin, const double* __restrict__ table_eval, int n, int tile_points,
                                                      double* __restrict__ partials, const int* __restrict__ corr) {
  static_assert(MODE == MODE_LIN_GENERAL || MODE == MODE_ERR, "a two-pose factor has no 29-sum form");
  constexpr int NREG = MODE == MODE_ERR ? 2 : ACCG_SIZE;
  double acc[NREG];
#pragma unroll
  for (int k = 0; k < NREG; k++) acc[k] = 0.0;
  const int begin = blockIdx.x * tile_points;
  const int end = min(begin + tile_points, n);
  if constexpr (MODE == MODE_ERR) {
    for (int i = begin + threadIdx.x; i < end; i += 256) {
      const int c = corr[i];
      if (c < 0) continue;
      const size_t b = (size_t)f.f.time_index[i];
      f.template accumulate<MODE>(i, (size_t)c, table_lin + b * kCtPoseRow, table_eval + b * kCtPoseRow, acc, nullptr);
    }
  } else {
    double loc[LOC_SIZE];
#pragma unroll
    for (int k = 0; k < LOC_SIZE; k++) loc[k] = 0.0;
    int cur = -1;  // the bin the local sums belong to
    // (one trip past the lane's last point: the bin still open is applied there, so the kernel holds ONE copy of ct_apply_bin)
    for (int i = begin + threadIdx.x;; i += 256) {
      int b = -1, c = -1;
      if (i < end) {
        c = corr[i];
        if (c >= 0) b = f.f.time_index[i];
      }
      if (b != cur) {
        if (cur >= 0) ct_apply_bin(table_lin + (size_t)cur * kCtPoseRow, loc, acc);
        cur = b;
      }
      if (i >= end) break;
      if (b >= 0) {
        const double* row = table_lin + (size_t)b * kCtPoseRow;
        f.template accumulate<MODE>(i, (size_t)c, row, row, acc, loc);
      }
    }
  }
  store_tile_sums<MODE>(acc, partials);
}

// deskewed_source_points (:290-308): T(t_i) p_i, or T0^-1 T(t_i) p_i, one point per lane
struct CtDeskew {
  double inv0[12];  // T0^-1 as a 3x4 row-major block
  int local;
};

__global__ void __launch_bounds__(256) ct_deskew_kernel(const float* __restrict__ points, const int* __restrict__ time_index, const double* __restrict__ table, int n,
                                                        const CtDeskew d, double* __restrict__ out) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const Pose T = load_pose_row(table + (size_t)time_index[i] * kCtPoseRow);
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  double qx = T.r00 * px + T.r01 * py + T.r02 * pz + T.tx;
  double qy = T.r10 * px + T.r11 * py + T.r12 * pz + T.ty;
  double qz = T.r20 * px + T.r21 * py + T.r22 * pz + T.tz;
  if (d.local) {
    const Pose I = load_pose_row(d.inv0);
    const double lx = I.r00 * qx + I.r01 * qy + I.r02 * qz + I.tx;
    const double ly = I.r10 * qx + I.r11 * qy + I.r12 * qz + I.ty;
    const double lz = I.r20 * qx + I.r21 * qy + I.r22 * qz + I.tz;
    qx = lx, qy = ly, qz = lz;
  }
  double* __restrict__ o = out + 4 * (size_t)i;
  o[0] = qx, o[1] = qy, o[2] = qz, o[3] = 1.0;
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

struct gp_ct_factor : gp_corr_factor_core {  // (the grid is BORROWED, as the ICP factor's)
  gp::CtDesc desc{};
  int kind = 0;
  std::vector<double> time_table;  // normalised
  std::vector<int> time_indices;
  gp::DeviceArray d_times, d_indices;   // double[bins], int[n]
  gp::DeviceArray table_lin, table_eval;  // double[bins][kCtPoseRow]: of the stored correspondences (T, D0, D1) / of the call in hand (T only)

  int bins() const { return (int)time_table.size(); }

  int pose_table(const double* pose0, const double* pose1, bool derivs, double* table) {
    if (bins() == 0) return GP_OK;
    gp::CtPoses P;
    memcpy(P.pose0, pose0, sizeof(double) * 16);
    memcpy(P.pose1, pose1, sizeof(double) * 16);
    hipLaunchKernelGGL(gp::ct_pose_table_kernel, dim3((bins() + 63) / 64), dim3(64), 0, stream, P, d_times.as<double>(), bins(), derivs ? 1 : 0, table);
    GP_HIP(hipGetLastError());
    return GP_OK;
  }

  // the linearisation pose table at (pose0, pose1) and the correspondences at its poses (n > 0)
  int search_at(const double* pose0, const double* pose1) {
    GP_TRY(pose_table(pose0, pose1, true, table_lin.as<double>()));
    gp::CtSearchDesc s;
    s.points = points;
    s.time_index = d_indices.as<int>();
    s.table = table_lin.as<double>();
    s.grid = grid->view();
    s.n = n;
    s.max_sq_dist = max_sq_dist;
    hipLaunchKernelGGL(gp::ct_nearest_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, s, corr.as<int>());
    GP_HIP(hipGetLastError());
    upd.corr_valid = true;  // (of the update rule, a two-pose factor keeps this one word: a linearise always searches, an error evaluation only when nothing is stored)
    return GP_OK;
  }

  template <int MODE, class TERM>
  void launch_tiles(const TERM& term) {
    hipLaunchKernelGGL((gp::ct_tile_kernel<MODE, TERM>), dim3(num_tiles), dim3(256), 0, stream, term, table_lin.as<double>(), table_eval.as<double>(), n, tile_points,
                       partials.as<double>(), corr.as<int>());
  }

  // one synchronous pass over the stored correspondences: a linearise (out_host a gp_linearized6) or the error at table_eval (out_host a double)
  int run(bool error, const double* pose0, void* out_host) {
    if (num_tiles > 0) {
      if (kind == 0) {
        if (error)
          launch_tiles<gp::MODE_ERR>(gp::CtIcpTerm{desc});
        else
          launch_tiles<gp::MODE_LIN_GENERAL>(gp::CtIcpTerm{desc});
      } else {
        if (error)
          launch_tiles<gp::MODE_ERR>(gp::CtGicpTerm{desc});
        else
          launch_tiles<gp::MODE_LIN_GENERAL>(gp::CtGicpTerm{desc});
      }
      GP_HIP(hipGetLastError());
    }
    return finish_pass(error, pose0, true, out_host);  // (a two-pose factor has the 92 sums only: pose0 is not read)
  }
};

// the time table of IntegratedCT_ICPFactor_'s constructor (:41-55), greedy and sequential, f64 on the f32 times
static void ct_build_time_table(const std::vector<float>& times, std::vector<double>* table, std::vector<int>* indices) {
  const double time_eps = 1e-3;
  table->clear();
  indices->clear();
  indices->reserve(times.size());
  for (const float tf : times) {
    const double t = (double)tf;
    if (table->empty() || t - table->back() > time_eps) table->push_back(t);
    indices->push_back((int)table->size() - 1);
  }
  if (table->empty()) return;
  const double last = std::max(1e-9, table->back());
  for (double& t : *table) t = t / last;
}

extern "C" {

int gp_ct_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, const float* target_covs_dev, int n_target,
                        const float* points_dev, const float* covs_dev, const float* times_dev, int n, double max_correspondence_distance_sq, int kind, gp_stream_t stream,
                        gp_ct_factor_t** out) {
  if (!grid || !target_points_dev || !points_dev || !times_dev || n < 0 || n_target < 0 || !(max_correspondence_distance_sq >= 0.0) || !out || (kind != 0 && kind != 1))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_create: bad arguments (a NULL grid, points or times, a negative count or cut-off, a kind that is not 0 or 1)");
  if (kind == 0 && !target_normals_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_create: a CT-ICP factor needs the target's normals");
  if (kind == 1 && (!target_covs_dev || !covs_dev)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_create: a CT-GICP factor needs the covariances of both clouds");
  auto f = std::make_unique<gp_ct_factor>();
  hipStream_t s = (hipStream_t)stream;
  f->kind = kind;
  GP_TRY(f->prepare(grid, points_dev, n, max_correspondence_distance_sq, s));
  std::vector<float> times((size_t)n);
  if (n > 0) {
    GP_HIP(hipMemcpyAsync(times.data(), times_dev, sizeof(float) * (size_t)n, hipMemcpyDeviceToHost, s));
    GP_HIP(hipStreamSynchronize(s));
  }
  ct_build_time_table(times, &f->time_table, &f->time_indices);
  const size_t bins = f->time_table.size();
  GP_TRY(f->d_times.alloc(sizeof(double) * std::max<size_t>(bins, 1)));
  GP_TRY(f->d_indices.alloc(sizeof(int) * (size_t)std::max(n, 1)));
  GP_TRY(f->table_lin.alloc(sizeof(double) * gp::kCtPoseRow * std::max<size_t>(bins, 1)));
  GP_TRY(f->table_eval.alloc(sizeof(double) * gp::kCtPoseRow * std::max<size_t>(bins, 1)));
  if (n > 0) {
    GP_HIP(hipMemcpyAsync(f->d_times.ptr, f->time_table.data(), sizeof(double) * bins, hipMemcpyHostToDevice, s));
    GP_HIP(hipMemcpyAsync(f->d_indices.ptr, f->time_indices.data(), sizeof(int) * (size_t)n, hipMemcpyHostToDevice, s));
    GP_HIP(hipStreamSynchronize(s));
  }
  f->desc = {points_dev, covs_dev, f->d_indices.as<int>(), target_points_dev, target_normals_dev, target_covs_dev};
  *out = f.release();
  return GP_OK;
}

int gp_ct_factor_destroy(gp_ct_factor_t* f) { return gp_corr_destroy(f); }  // (the grid is the caller's)

// update_poses + update_correspondences + the sums (:132-199): a linearise always searches
int gp_ct_factor_linearize(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], gp_linearized6* out_host) {
  if (!f || !pose0 || !pose1 || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_linearize: null");
  if (f->num_tiles > 0) GP_TRY(f->search_at(pose0, pose1));
  GP_TRY(f->run(false, pose0, out_host));
  f->num_inliers = (int)out_host->num_inliers;
  return GP_OK;
}

// error() (:92-129; ct_gicp :64-100): the pose table at the given poses, the stored correspondences -- and for GICP the stored pose table for M -- unless none are
int gp_ct_factor_compute_error(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], double* out_host) {
  if (!f || !pose0 || !pose1 || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_compute_error: null");
  if (f->num_tiles > 0) {
    if (!f->upd.corr_valid) GP_TRY(f->search_at(pose0, pose1));
    GP_TRY(f->pose_table(pose0, pose1, false, f->table_eval.as<double>()));
  }
  return f->run(true, pose0, out_host);
}

int gp_ct_factor_deskew(gp_ct_factor_t* f, const double pose0[16], const double pose1[16], int local, double* out_dev) {
  if (!f || !pose0 || !pose1 || (!out_dev && f->n > 0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_deskew: null");
  if (f->n == 0) return GP_OK;
  GP_TRY(f->pose_table(pose0, pose1, false, f->table_eval.as<double>()));
  gp::CtDeskew d;
  for (int r = 0; r < 3; r++) {  // T0^-1 = (R^T, -R^T t) of the column-major pose0
    for (int c = 0; c < 3; c++) d.inv0[4 * r + c] = pose0[4 * r + c];
    d.inv0[4 * r + 3] = -(pose0[4 * r] * pose0[12] + pose0[4 * r + 1] * pose0[13] + pose0[4 * r + 2] * pose0[14]);
  }
  d.local = local != 0;
  hipLaunchKernelGGL(gp::ct_deskew_kernel, dim3((f->n + 255) / 256), dim3(256), 0, f->stream, f->points, f->d_indices.as<int>(), f->table_eval.as<double>(), f->n, d, out_dev);
  GP_HIP(hipGetLastError());
  GP_HIP(hipStreamSynchronize(f->stream));
  return GP_OK;
}

int gp_ct_factor_num_time_bins(const gp_ct_factor_t* f) { return f ? f->bins() : 0; }

int gp_ct_factor_time_table(const gp_ct_factor_t* f, double* table_host, int* indices_host) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_time_table: null");
  if (table_host && f->bins() > 0) memcpy(table_host, f->time_table.data(), sizeof(double) * f->time_table.size());
  if (indices_host && f->n > 0) memcpy(indices_host, f->time_indices.data(), sizeof(int) * f->time_indices.size());
  return GP_OK;
}

int gp_ct_factor_pose_table(gp_ct_factor_t* f, double* out_host) {
  if (!f || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_pose_table: null");
  if (f->n == 0) return GP_OK;
  if (!f->upd.corr_valid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_pose_table: no linearise or error evaluation yet");
  GP_HIP(hipMemcpyAsync(out_host, f->table_lin.ptr, sizeof(double) * gp::kCtPoseRow * (size_t)f->bins(), hipMemcpyDeviceToHost, f->stream));
  GP_HIP(hipStreamSynchronize(f->stream));
  return GP_OK;
}

int gp_ct_factor_correspondences(gp_ct_factor_t* f, int* out_host) {
  if (!f || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_correspondences: null");
  if (f->n == 0) return GP_OK;
  if (!f->upd.corr_valid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_ct_factor_correspondences: no linearise or error evaluation yet");
  GP_HIP(hipMemcpyAsync(out_host, f->corr.ptr, sizeof(int) * (size_t)f->n, hipMemcpyDeviceToHost, f->stream));
  GP_HIP(hipStreamSynchronize(f->stream));
  return GP_OK;
}

}  // extern "C"
