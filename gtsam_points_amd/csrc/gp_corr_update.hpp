// gp_corr_update.hpp -- which pose the stored correspondences of a matching-cost factor belong to, and the three decisions taken on it: written once for the GICP,
// ICP, colored GICP and LOAM factors (gp_corr_factors.hpp).  Host code on the standard library alone -- no HIP header -- so that a host compiler builds it by itself
// (tests/corr_update_cases.cpp, run under the sanitizers by tests/test_corr_update_cpu.py).
#pragma once
#include <cmath>
#include <cstring>

struct gp_corr_update {
  double corr_pose[16] = {0};  // last_correspondence_point: the pose the stored correspondences were searched at
  bool corr_valid = false;
  double lin_pose[16] = {0};  // the pose of the last linearise (which may have kept older correspondences: the update tolerances)
  bool lin_valid = false;
  double tol_rot = 0.0, tol_trans = 0.0;  // correspondence_update_tolerance_rot / _trans (integrated_icp_factor_impl.hpp:32-33); GICP leaves them zero

  static bool same_pose(const double* a, const double* b) { return memcmp(a, b, sizeof(double) * 16) == 0; }

  // update_correspondences' decision (integrated_icp_factor_impl.hpp:129-137, integrated_loam_factor_impl.hpp:81-88, :236-243, integrated_colored_gicp_factor_impl.hpp
  // :103-110) for a linearise at the column-major 4x4 `delta`: diff = delta^-1 * corr_pose (the isometry inverse, R^T and -R^T t), its rotation angle and the norm of
  // its translation against the tolerances, both strict.  false: search again.
  bool keep(const double* delta) const {
    if (!corr_valid || !(tol_trans > 0.0 || tol_rot > 0.0)) return false;
    const double* last = corr_pose;
    double D[3][3], t[3];
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) D[r][c] = delta[4 * r] * last[4 * c] + delta[4 * r + 1] * last[4 * c + 1] + delta[4 * r + 2] * last[4 * c + 2];
      t[r] = delta[4 * r] * (last[12] - delta[12]) + delta[4 * r + 1] * (last[13] - delta[13]) + delta[4 * r + 2] * (last[14] - delta[14]);
    }
    // angle in [0, pi] from sin (the skew part) and cos (the trace): what Eigen::AngleAxisd(diff.linear()).angle() gives for a rotation
    const double sx = 0.5 * (D[2][1] - D[1][2]), sy = 0.5 * (D[0][2] - D[2][0]), sz = 0.5 * (D[1][0] - D[0][1]);
    const double diff_rot = std::atan2(std::sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (D[0][0] + D[1][1] + D[2][2] - 1.0));
    const double diff_trans = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
    return diff_rot < tol_rot && diff_trans < tol_trans;
  }

  // an error evaluation with this pose_lin: the stored correspondences serve when it is the pose of the last linearise (which may itself have kept older ones) or
  // the pose they were searched at.  false: search at pose_lin.
  bool stored(const double* pose_lin) const { return corr_valid && ((lin_valid && same_pose(lin_pose, pose_lin)) || same_pose(corr_pose, pose_lin)); }

  // a search at `pose` has been issued: the correspondences are its own, and no linearise stands behind them until note_linearize says so
  void note_search(const double* pose) {
    memcpy(corr_pose, pose, sizeof(double) * 16);
    corr_valid = true;
    lin_valid = false;
  }

  // a linearise at `pose`, on kept or on fresh correspondences
  void note_linearize(const double* pose) {
    memcpy(lin_pose, pose, sizeof(double) * 16);
    lin_valid = true;
  }
};
