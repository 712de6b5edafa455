// gp_colored_factors.hip -- the colored GICP factor on nearest-neighbour correspondences and the intensity gradients it reads.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/intensity_gradients.cpp:20-133                               IntensityGradients::estimate  -> gp_estimate_intensity_gradients*
//   factors/impl/integrated_colored_gicp_factor_impl.hpp:101-253         correspondences + H/b         -> gp_colored_gicp_factor_*
//
// The factor is one more term on the correspondence core (gp_corr_tile.hpp): gp::launch_nearest_correspondences writes the nearest target point of every source
// point, the tile kernel sums the term over them into the partial-row layout of the VGICP factor (gp_device.hpp ACC / ACCG), the VGICP finalize kernels expand
// the rows.  The one difference to the other terms is that the photometric residual adds a rank-one part to both M and the right-hand side, so the sums are fed
// with (M, w, error) instead of (M, d): see accumulate_sums_mw.
#include <limits>

#include "gp_corr_tile.hpp"

namespace gp {

// accumulate_sums (gp_vgicp_shared.hpp) for a term whose right-hand side is not M d: given M (6, symmetric), w and the term's error, the sums of
// H = sum J^T M J, b = sum J^T w with J_t = [-[q]x, I], J_s = [R [p]x, -R], in the same slots -- ACC_QXMR / ACC_MR and ACCG_BS take w where accumulate_sums puts
// M r, ACC_ERR takes `err`.  The 29-sum rigid path and its adjoint finalize only use H = J^T M J, b = J^T w and J_s = -J_t Ad, so they serve unchanged.
template <int MODE>
__device__ __forceinline__ void accumulate_sums_mw(const Pose& Tl, const double* m, double wx, double wy, double wz, double err, double px, double py, double pz,
                                                   double qx, double qy, double qz, double* acc) {
  acc[ACC_COUNT] += 1.0;
  acc[ACC_ERR] += err;
  if constexpr (MODE != MODE_ERR) {
    for (int k = 0; k < 6; k++) acc[ACC_M + k] += m[k];
    // K = M [q]x, row-major
    const double Kf[3][3] = {{m[1] * qz - m[2] * qy, m[2] * qx - m[0] * qz, m[0] * qy - m[1] * qx},
                             {m[3] * qz - m[4] * qy, m[4] * qx - m[1] * qz, m[1] * qy - m[3] * qx},
                             {m[4] * qz - m[5] * qy, m[5] * qx - m[2] * qz, m[2] * qy - m[4] * qx}};
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) acc[ACC_K + 3 * r + c] += Kf[r][c];
    // TL = -[q]x K (= [q]x^T M [q]x), upper triangle
    acc[ACC_TL + 0] += qz * Kf[1][0] - qy * Kf[2][0];
    acc[ACC_TL + 1] += qz * Kf[1][1] - qy * Kf[2][1];
    acc[ACC_TL + 2] += qz * Kf[1][2] - qy * Kf[2][2];
    acc[ACC_TL + 3] += qx * Kf[2][1] - qz * Kf[0][1];
    acc[ACC_TL + 4] += qx * Kf[2][2] - qz * Kf[0][2];
    acc[ACC_TL + 5] += qy * Kf[0][2] - qx * Kf[1][2];
    // b_t = [q x w; w]
    acc[ACC_QXMR + 0] += qy * wz - qz * wy;
    acc[ACC_QXMR + 1] += qz * wx - qx * wz;
    acc[ACC_QXMR + 2] += qx * wy - qy * wx;
    acc[ACC_MR + 0] += wx;
    acc[ACC_MR + 1] += wy;
    acc[ACC_MR + 2] += wz;

    if constexpr (MODE == MODE_LIN_GENERAL) {
      // explicit source side: J_s = [R [p]x, -R] with R the block as given
      const double Mf[3][3] = {{m[0], m[1], m[2]}, {m[1], m[3], m[4]}, {m[2], m[4], m[5]}};
      const double Rf[3][3] = {{Tl.r00, Tl.r01, Tl.r02}, {Tl.r10, Tl.r11, Tl.r12}, {Tl.r20, Tl.r21, Tl.r22}};
      double Js[3][6], JtM[6][3], JsM[6][3];
#pragma unroll
      for (int r = 0; r < 3; r++) {
        Js[r][0] = Rf[r][1] * pz - Rf[r][2] * py;
        Js[r][1] = Rf[r][2] * px - Rf[r][0] * pz;
        Js[r][2] = Rf[r][0] * py - Rf[r][1] * px;
#pragma unroll
        for (int c = 0; c < 3; c++) {
          Js[r][3 + c] = -Rf[r][c];
          JtM[r][c] = -Kf[c][r];  // J_t^T M = [[q]x M; M] = [-K^T; M]
          JtM[3 + r][c] = Mf[r][c];
        }
      }
#pragma unroll
      for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) JsM[r][c] = Js[0][r] * Mf[0][c] + Js[1][r] * Mf[1][c] + Js[2][r] * Mf[2][c];
      // H_s = (J_s^T M) J_s in the ACCG order: TL (upper), BL (3..5 x 0..2), BR (upper)
      int idx = ACCG_HS_TL;
#pragma unroll
      for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = r; c < 3; c++) acc[idx++] += JsM[r][0] * Js[0][c] + JsM[r][1] * Js[1][c] + JsM[r][2] * Js[2][c];
#pragma unroll
      for (int r = 3; r < 6; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) acc[idx++] += JsM[r][0] * Js[0][c] + JsM[r][1] * Js[1][c] + JsM[r][2] * Js[2][c];
#pragma unroll
      for (int r = 3; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) acc[idx++] += JsM[r][0] * Js[0][c] + JsM[r][1] * Js[1][c] + JsM[r][2] * Js[2][c];
      static_assert(ACCG_HS_BL == ACCG_HS_TL + 6 && ACCG_HS_BR == ACCG_HS_BL + 9 && ACCG_HTS == ACCG_HS_BR + 6, "the three parts of H_s are contiguous");
      // H_ts = (J_t^T M) J_s, row-major; b_s = J_s^T w
#pragma unroll
      for (int r = 0; r < 6; r++) {
#pragma unroll
        for (int c = 0; c < 6; c++) acc[ACCG_HTS + 6 * r + c] += JtM[r][0] * Js[0][c] + JtM[r][1] * Js[1][c] + JtM[r][2] * Js[2][c];
        acc[ACCG_BS + r] += Js[0][r] * wx + Js[1][r] * wy + Js[2][r] * wz;
      }
    }
  }
}

// The per-point body of IntegratedColoredGICPFactor_::evaluate (integrated_colored_gicp_factor_impl.hpp:183-252) in the project's signs (d = mu_B - q and
// J_t = [-[q]x, I]; the reference has q - mu_B and -J_t, :203, :217-223: the products are the same):
//   q = T p_A, d = mu_B - q, M_g = (C_B + R C_A R^T)^-1 at the LINEARISATION pose (:134-138: stored by update_correspondences, not recomputed by error()),
//   P = I - n_B n_B^T, u = P g_B (:236-241), r_p = I_B - I_A - u . d (:207-209), w_p = photometric_term_weight, w_g = 1 - w_p (:174),
//   error = w_g d^T M_g d + w_p r_p^2 (:204, :211), M = w_g M_g + w_p u u^T (:229, :246), w = w_g M_g d - w_p r_p u (:232, :249).
// A matched point costs 132 B: 4 (index) + 12 + 36 + 4 (source point, covariance, intensity) + 12 + 36 + 12 + 4 + 12 (target point, covariance, normal,
// intensity, gradient), against the GICP term's 100 B.
struct ColoredGicpTerm {
  const float* points;
  const float* covs;
  const float* intensities;
  const float* target_points;
  const float* target_covs;
  const float* target_normals;
  const float* target_intensities;
  const float* target_gradients;
  double photometric_term_weight;
  static constexpr int kErrRegs = 2;
  static constexpr int kNeighbours = 1;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const Pose& Tl, const Pose& Te, double* acc) const {
    const ColoredGicpTerm& f = *this;
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    const double qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    const double qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
    const float* cp = f.covs + 9 * (size_t)i;
    const float* cq = f.target_covs + 9 * j;
    // symmetric parts of both column-major 3x3 covariances, as the GICP term takes them
    const double ca[6] = {(double)cp[0], 0.5 * ((double)cp[3] + (double)cp[1]), 0.5 * ((double)cp[6] + (double)cp[2]),
                          (double)cp[4], 0.5 * ((double)cp[7] + (double)cp[5]), (double)cp[8]};
    const double cb[6] = {(double)cq[0], 0.5 * ((double)cq[3] + (double)cq[1]), 0.5 * ((double)cq[6] + (double)cq[2]),
                          (double)cq[4], 0.5 * ((double)cq[7] + (double)cq[5]), (double)cq[8]};
    double mg[6];
    fused_mahalanobis(Tl, ca, cb, mg);
    const double dx = (double)f.target_points[3 * j] - qx, dy = (double)f.target_points[3 * j + 1] - qy, dz = (double)f.target_points[3 * j + 2] - qz;
    const double nx = (double)f.target_normals[3 * j], ny = (double)f.target_normals[3 * j + 1], nz = (double)f.target_normals[3 * j + 2];
    const double gx = (double)f.target_gradients[3 * j], gy = (double)f.target_gradients[3 * j + 1], gz = (double)f.target_gradients[3 * j + 2];
    const double ng = nx * gx + ny * gy + nz * gz;
    const double ux = gx - ng * nx, uy = gy - ng * ny, uz = gz - ng * nz;
    const double rp = ((double)f.target_intensities[j] - (double)f.intensities[i]) - (ux * dx + uy * dy + uz * dz);
    const double wp = f.photometric_term_weight, wg = 1.0 - wp;
    const double mdx = mg[0] * dx + mg[1] * dy + mg[2] * dz;
    const double mdy = mg[1] * dx + mg[3] * dy + mg[4] * dz;
    const double mdz = mg[2] * dx + mg[4] * dy + mg[5] * dz;
    const double err = wg * (dx * mdx + dy * mdy + dz * mdz) + wp * (rp * rp);
    const double m[6] = {wg * mg[0] + wp * (ux * ux), wg * mg[1] + wp * (ux * uy), wg * mg[2] + wp * (ux * uz),
                         wg * mg[3] + wp * (uy * uy), wg * mg[4] + wp * (uy * uz), wg * mg[5] + wp * (uz * uz)};
    const double s = wp * rp;
    accumulate_sums_mw<MODE>(Tl, m, wg * mdx - s * ux, wg * mdy - s * uy, wg * mdz - s * uz, err, px, py, pz, qx, qy, qz, acc);
  }
};

// IntensityGradients::estimate (intensity_gradients.cpp:40-66), one point per lane, f64 on the f32 inputs: rows of A are the normal (b = 0) and, for the slots
// 1 .. k_photo - 1 of the point's neighbour list (slot 0 is the point itself and is skipped, :54), the neighbour projected onto the tangent plane minus the point
// with b = I_j - I; H = A^T A, e = A^T b, g = H^-1 e with the cofactor inverse, rounded once at the store.  The hot part is the gather of k_photo x 16 B.
// A slot among the first k_photo that is no point index (the search's -1 padding; anything outside [0, n) is refused the same way) gives (0, 0, 0) and counts
// in *num_short.  A singular H is not guarded: its non-finite values are stored.
__global__ void __launch_bounds__(256) intensity_gradient_kernel(const float* __restrict__ points, const float* __restrict__ normals, const float* __restrict__ intensities,
                                                                 int n, const int* __restrict__ neighbors, int k, int k_photo, float* __restrict__ gradients,
                                                                 int* __restrict__ num_short) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* __restrict__ nb = neighbors + (size_t)i * (size_t)k;
  bool ok = true;
  for (int j = 0; j < k_photo; j++) ok = ok && (unsigned)nb[j] < (unsigned)n;
  float* __restrict__ out = gradients + 3 * (size_t)i;
  if (!ok) {
    out[0] = out[1] = out[2] = 0.0f;
    if (num_short) atomicAdd(num_short, 1);
    return;
  }
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  const double nx = (double)normals[3 * (size_t)i], ny = (double)normals[3 * (size_t)i + 1], nz = (double)normals[3 * (size_t)i + 2];
  const double intensity = (double)intensities[i];
  double h00 = nx * nx, h01 = nx * ny, h02 = nx * nz, h11 = ny * ny, h12 = ny * nz, h22 = nz * nz;  // row 0 of A: the normal
  double e0 = 0.0, e1 = 0.0, e2 = 0.0;
  for (int j = 1; j < k_photo; j++) {
    const size_t t = (size_t)nb[j];
    const double tx = (double)points[3 * t], ty = (double)points[3 * t + 1], tz = (double)points[3 * t + 2];
    const double b = (double)intensities[t] - intensity;
    const double along = (tx - px) * nx + (ty - py) * ny + (tz - pz) * nz;
    const double ax = (tx - along * nx) - px, ay = (ty - along * ny) - py, az = (tz - along * nz) - pz;
    h00 += ax * ax;
    h01 += ax * ay;
    h02 += ax * az;
    h11 += ay * ay;
    h12 += ay * az;
    h22 += az * az;
    e0 += ax * b;
    e1 += ay * b;
    e2 += az * b;
  }
  double hi[6];
  inverse_sym3(h00, h01, h02, h11, h12, h22, hi);
  out[0] = (float)(hi[0] * e0 + hi[1] * e1 + hi[2] * e2);
  out[1] = (float)(hi[1] * e0 + hi[3] * e1 + hi[4] * e2);
  out[2] = (float)(hi[2] * e0 + hi[4] * e1 + hi[5] * e2);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

struct gp_colored_gicp_factor : gp_corr_factor_core {  // (the grid is BORROWED, as the ICP factor's)
  gp::ColoredGicpTerm term{};
  double lin_pose[16] = {0};  // the pose of the last linearise (which may have kept older correspondences: the update tolerances)
  bool lin_valid = false;
  double tol_rot = 0.0, tol_trans = 0.0;  // correspondence_update_tolerance_rot / _trans (:103-110)
  int num_correspondences = 0;
};

extern "C" {

// ---- intensity gradients ----------------------------------------------------------------------------------------------

int gp_estimate_intensity_gradients_from_neighbors(const float* points_dev, const float* normals_dev, const float* intensities_dev, int n, const int* neighbors_dev, int k,
                                                   int k_photo, float* gradients_dev, gp_stream_t stream) {
  if (!points_dev || !normals_dev || !intensities_dev || !neighbors_dev || !gradients_dev || n < 0 || k < 1 || k_photo < 1 || k_photo > k)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_intensity_gradients_from_neighbors: bad arguments (no NULL array, n >= 0, 1 <= k_photo <= k)");
  if (n == 0) return GP_OK;
  hipLaunchKernelGGL(gp::intensity_gradient_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, points_dev, normals_dev, intensities_dev, n, neighbors_dev, k,
                     k_photo, gradients_dev, static_cast<int*>(nullptr));
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_estimate_intensity_gradients(const float* points_dev, const float* normals_dev, const float* intensities_dev, int n, int k, double cell_size, float* gradients_dev,
                                    int* num_short, gp_stream_t stream) {
  if (!points_dev || !normals_dev || !intensities_dev || !gradients_dev || n < 0 || k < 1 || k > 32)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_intensity_gradients: bad arguments (no NULL array, n >= 0, 1 <= k <= 32)");
  if (num_short) *num_short = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  struct Grid {
    gp_point_grid_t* g = nullptr;
    ~Grid() {
      if (g) gp_point_grid_destroy(g);
    }
  } grid;
  GP_TRY(gp_point_grid_create(points_dev, n, cell_size > 0.0 ? cell_size : 0.25, stream, &grid.g));
  gp::DeviceArray table, counter;  // int[n][k] neighbour lists; the number of points with fewer than k
  GP_TRY(table.alloc_async(sizeof(int) * (size_t)n * (size_t)k, s));
  GP_TRY(counter.alloc_async(sizeof(int), s));
  GP_HIP(hipMemsetAsync(counter.ptr, 0, sizeof(int), s));
  GP_TRY(gp_knn_search(grid.g, points_dev, n, k, std::numeric_limits<double>::max(), table.as<int>(), nullptr, nullptr, stream));
  hipLaunchKernelGGL(gp::intensity_gradient_kernel, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, normals_dev, intensities_dev, n, table.as<int>(), k, k, gradients_dev,
                     counter.as<int>());
  GP_HIP(hipGetLastError());
  int h_short = 0;
  GP_HIP(hipMemcpyAsync(&h_short, counter.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));  // (also: the search has finished with the grid before it goes)
  if (num_short) *num_short = h_short;
  return GP_OK;
}

// ---- colored GICP factor ----------------------------------------------------------------------------------------------

int gp_colored_gicp_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_covs_dev, const float* target_normals_dev,
                                  const float* target_intensities_dev, const float* target_gradients_dev, int n_target, const float* points_dev, const float* covs_dev,
                                  const float* intensities_dev, int n, double max_correspondence_distance_sq, double photometric_term_weight, gp_stream_t stream,
                                  gp_colored_gicp_factor_t** out) {
  if (!grid || !target_points_dev || !target_covs_dev || !target_normals_dev || !target_intensities_dev || !target_gradients_dev || !points_dev || !covs_dev ||
      !intensities_dev || n < 0 || n_target < 0 || !(max_correspondence_distance_sq > 0.0) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_create: bad arguments (a NULL grid or array, a negative count, a cut-off that is not positive)");
  if (!(photometric_term_weight >= 0.0 && photometric_term_weight <= 1.0))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_create: photometric_term_weight outside [0, 1]");
  auto f = std::make_unique<gp_colored_gicp_factor>();
  f->term = {points_dev,         covs_dev,        intensities_dev,       target_points_dev, target_covs_dev, target_normals_dev, target_intensities_dev,
             target_gradients_dev, photometric_term_weight};
  GP_TRY(f->prepare(grid, points_dev, n, max_correspondence_distance_sq, (hipStream_t)stream));
  *out = f.release();
  return GP_OK;
}

int gp_colored_gicp_factor_destroy(gp_colored_gicp_factor_t* f) {
  if (!f) return GP_OK;
  (void)hipStreamSynchronize(f->stream);
  delete f;  // (the grid is the caller's)
  return GP_OK;
}

int gp_colored_gicp_factor_set_photometric_term_weight(gp_colored_gicp_factor_t* f, double weight) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_photometric_term_weight: null");
  if (!(weight >= 0.0 && weight <= 1.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_photometric_term_weight: weight outside [0, 1]");
  f->term.photometric_term_weight = weight;
  return GP_OK;
}

int gp_colored_gicp_factor_set_max_correspondence_distance(gp_colored_gicp_factor_t* f, double dist) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_max_correspondence_distance: null");
  if (!(dist > 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_max_correspondence_distance: the distance must be positive");
  f->max_sq_dist = dist * dist;
  return GP_OK;
}

int gp_colored_gicp_factor_set_correspondence_update_tolerance(gp_colored_gicp_factor_t* f, double angle, double trans) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_correspondence_update_tolerance: null");
  f->tol_rot = angle;
  f->tol_trans = trans;
  return GP_OK;
}

int gp_colored_gicp_factor_num_correspondences(const gp_colored_gicp_factor_t* f) { return f ? f->num_correspondences : 0; }

int gp_colored_gicp_factor_linearize(gp_colored_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_linearize: null");
  if (f->num_tiles > 0 && !keep_correspondences(f->corr_valid, f->corr_pose, f->tol_rot, f->tol_trans, pose)) GP_TRY(f->search(pose));
  memcpy(f->lin_pose, pose, sizeof(double) * 16);
  f->lin_valid = true;
  GP_TRY(f->run_pass(f->term, pose, nullptr, out_host));
  f->num_correspondences = (int)out_host->num_inliers;
  return GP_OK;
}

int gp_colored_gicp_factor_compute_error(gp_colored_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_compute_error: null");
  // the stored correspondences serve when pose_lin is the pose of the last linearise (which may itself have kept older ones) or the pose they were searched at
  const bool stored = f->corr_valid && ((f->lin_valid && memcmp(f->lin_pose, pose_lin, sizeof(double) * 16) == 0) || f->searched_at(pose_lin));
  if (f->num_tiles > 0 && !stored) {
    GP_TRY(f->search(pose_lin));
    f->lin_valid = false;
  }
  return f->run_pass(f->term, pose_lin, pose_eval, out_host);
}

}  // extern "C"
