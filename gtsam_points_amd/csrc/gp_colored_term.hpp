// gp_colored_term.hpp -- what the colored GICP factor's single-factor entry points (gp_colored_factors.hip) share with the correspondence batch (gp_corr_batch.hip): the
// per-point term, the sums it feeds, and the factor handle the batch borrows.
#pragma once
#include "gp_corr_factors.hpp"

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

// The per-point body of IntegratedColorConsistencyFactor_::evaluate (integrated_color_consistency_factor_impl.hpp:176-222) in the project's signs: the colored term's
// photometric part alone,
//   q = T p_A, d = mu_B - q, u = (I - n_B n_B^T) g_B (:207-215), r_p = I_B - I_A - u . d (:195-198: I_B + g_B . (projected - mu_B) - I_A, projected - mu_B = -P d),
//   w = photometric_term_weight (default 1.0, :31): error = w r_p^2 (:200), M = w u u^T (:217-219), the vector handed to accumulate_sums_mw is -w r_p u (:220-221).
// That is ColoredGicpTerm at w_g = 0 without the Mahalanobis matrix: no covariance is read and nothing is inverted.  A matched point costs 60 B: 4 (index) + 12 + 4
// (source point, intensity) + 12 + 12 + 4 + 12 (target point, normal, intensity, gradient).
struct ColorConsistencyTerm {
  const float* points;
  const float* intensities;
  const float* target_points;
  const float* target_normals;
  const float* target_intensities;
  const float* target_gradients;
  double photometric_term_weight;
  static constexpr int kErrRegs = 2;
  static constexpr int kNeighbours = 1;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const Pose& Tl, const Pose& Te, double* acc) const {
    const ColorConsistencyTerm& f = *this;
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    const double qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    const double qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
    const double dx = (double)f.target_points[3 * j] - qx, dy = (double)f.target_points[3 * j + 1] - qy, dz = (double)f.target_points[3 * j + 2] - qz;
    const double nx = (double)f.target_normals[3 * j], ny = (double)f.target_normals[3 * j + 1], nz = (double)f.target_normals[3 * j + 2];
    const double gx = (double)f.target_gradients[3 * j], gy = (double)f.target_gradients[3 * j + 1], gz = (double)f.target_gradients[3 * j + 2];
    const double ng = nx * gx + ny * gy + nz * gz;
    const double ux = gx - ng * nx, uy = gy - ng * ny, uz = gz - ng * nz;
    const double rp = ((double)f.target_intensities[j] - (double)f.intensities[i]) - (ux * dx + uy * dy + uz * dz);
    const double w = f.photometric_term_weight;
    const double m[6] = {w * (ux * ux), w * (ux * uy), w * (ux * uz), w * (uy * uy), w * (uy * uz), w * (uz * uz)};
    const double s = w * rp;
    accumulate_sums_mw<MODE>(Tl, m, -s * ux, -s * uy, -s * uz, w * (rp * rp), px, py, pz, qx, qy, qz, acc);
  }
};

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side: the factor handles
// ---------------------------------------------------------------------------------------------------------------

struct gp_colored_gicp_factor : gp_corr_factor_core {  // (the grid is BORROWED, as the ICP factor's)
  gp::ColoredGicpTerm term{};
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host);  // (gp_colored_factors.hip)
};

struct gp_color_consistency_factor : gp_corr_factor_core {  // (the grid is BORROWED)
  gp::ColorConsistencyTerm term{};
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host);  // (gp_color_consistency.hip)
};

// gp_*_factor_set_intensity_grid of the two photometric factors: from now on the correspondence pass is the XYZI search on `xyzi` (NULL: back to the 3-D grid).
// Stored correspondences are forgotten: they belong to the other search.
inline int gp_corr_set_intensity_grid(gp_corr_factor_core* f, const gp_intensity_grid* xyzi, const float* source_intensities, const char* who) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": null");
  f->xyzi = xyzi;
  f->intensities = source_intensities;
  f->upd.corr_valid = f->upd.lin_valid = false;
  return GP_OK;
}
