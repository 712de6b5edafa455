// gp_pose_factors.hpp -- gtsam::BetweenFactor<Pose3> and gtsam::PriorFactor<Pose3> with a Gaussian noise model, linearised into gp_linearized6 records on the device
// (gp_pose_factors.hip).  The formulas are GTSAM 4.2's in its default build (GTSAM_POSE3_EXPMAP on, GTSAM_SLOW_BUT_CORRECT_BETWEENFACTOR off), f64 throughout:
//   between (a, b, Z):  hx = T_a^-1 T_b,  e = Logmap(Z^-1 hx),  J_a = -AdjointMap(hx^-1),  J_b = I   (BetweenFactor::evaluateError: the Jacobians do NOT carry
//                       LogmapDerivative(e), as GTSAM's do not)
//   prior (a, Z):       e = Logmap(Z^-1 T_a),  J_a = I                                            (PriorFactor::evaluateError)
//   Gaussian:           error() = 1/2 e^T Lambda e;  H = J^T Lambda J,  b = J^T Lambda e  (the record's convention: g = -b)
// The pose algebra (Rigid, load_rigid, between_rigid) is the LM graph's own (gp_lm_poses.hpp).
#pragma once
#include <hip/hip_runtime.h>

#include "gp_lm_poses.hpp"

namespace gp {

// gtsam::SO3::Logmap (so3.cpp, GTSAM 4.2) of a row-major rotation, its three branches as written there
__device__ __forceinline__ void so3_logmap(const double* __restrict__ R, double* __restrict__ w) {
  const double R11 = R[0], R12 = R[1], R13 = R[2];
  const double R21 = R[3], R22 = R[4], R23 = R[5];
  const double R31 = R[6], R32 = R[7], R33 = R[8];
  const double tr = R11 + R22 + R33;
  if (tr + 1.0 < 1e-3) {  // theta near pi: from the largest diagonal entry
    double W, Q1, Q2, Q3;
    int order;
    if (R33 > R22 && R33 > R11) {
      W = R21 - R12, Q1 = 2.0 + 2.0 * R33, Q2 = R31 + R13, Q3 = R23 + R32, order = 2;
    } else if (R22 > R11) {
      W = R13 - R31, Q1 = 2.0 + 2.0 * R22, Q2 = R23 + R32, Q3 = R12 + R21, order = 1;
    } else {
      W = R32 - R23, Q1 = 2.0 + 2.0 * R11, Q2 = R12 + R21, Q3 = R31 + R13, order = 0;
    }
    const double r = sqrt(Q1), one_over_r = 1.0 / r;
    const double norm = sqrt(Q1 * Q1 + Q2 * Q2 + Q3 * Q3 + W * W);
    const double sgn_w = W < 0.0 ? -1.0 : 1.0;
    const double mag = M_PI - (2.0 * sgn_w * W) / norm;
    const double scale = 0.5 * one_over_r * mag;
    const double s = sgn_w * scale;
    if (order == 2) {
      w[0] = s * Q2, w[1] = s * Q3, w[2] = s * Q1;
    } else if (order == 1) {
      w[0] = s * Q3, w[1] = s * Q1, w[2] = s * Q2;
    } else {
      w[0] = s * Q1, w[1] = s * Q2, w[2] = s * Q3;
    }
    return;
  }
  const double tr_3 = tr - 3.0;
  double magnitude;
  if (tr_3 < -1e-6) {
    const double theta = acos((tr - 1.0) / 2.0);
    magnitude = theta / (2.0 * sin(theta));
  } else {  // theta near 0: the series of GTSAM issue 746
    magnitude = 0.5 - tr_3 / 12.0 + tr_3 * tr_3 / 60.0;
  }
  w[0] = magnitude * (R32 - R23), w[1] = magnitude * (R13 - R31), w[2] = magnitude * (R21 - R12);
}

// gtsam::Pose3::Logmap (pose3.cpp, GTSAM 4.2): xi = (omega, u)
__device__ __forceinline__ void pose3_logmap(const Rigid& T, double* __restrict__ xi) {
  double w[3];
  so3_logmap(T.R, w);
  const double t = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  xi[0] = w[0], xi[1] = w[1], xi[2] = w[2];
  if (t < 1e-10) {
    xi[3] = T.t[0], xi[4] = T.t[1], xi[5] = T.t[2];
    return;
  }
  const double n[3] = {w[0] / t, w[1] / t, w[2] / t};  // W = skew(w / t)
  const double WT[3] = {n[1] * T.t[2] - n[2] * T.t[1], n[2] * T.t[0] - n[0] * T.t[2], n[0] * T.t[1] - n[1] * T.t[0]};
  const double WWT[3] = {n[1] * WT[2] - n[2] * WT[1], n[2] * WT[0] - n[0] * WT[2], n[0] * WT[1] - n[1] * WT[0]};
  const double Tan = tan(0.5 * t);
  const double h = 0.5 * t, k = 1.0 - t / (2.0 * Tan);
  for (int i = 0; i < 3; i++) xi[3 + i] = T.t[i] - h * WT[i] + k * WWT[i];
}

// entry (r, c) of gtsam::Pose3::AdjointMap(T) in (omega, v) order: [[R, 0], [skew(t) R, R]]
__device__ __forceinline__ double adjoint(const Rigid& T, int r, int c) {
  if (r < 3) return c < 3 ? T.R[r * 3 + c] : 0.0;
  if (c >= 3) return T.R[(r - 3) * 3 + (c - 3)];
  const int i = r - 3;
  const double s[9] = {0.0, -T.t[2], T.t[1], T.t[2], 0.0, -T.t[0], -T.t[1], T.t[0], 0.0};  // skew(t), row-major
  return s[i * 3] * T.R[c] + s[i * 3 + 1] * T.R[3 + c] + s[i * 3 + 2] * T.R[6 + c];
}

// T^-1 = (R^T, -R^T t)
__device__ __forceinline__ Rigid inverse_rigid(const Rigid& T) {
  Rigid I;
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) I.R[r * 3 + c] = T.R[c * 3 + r];
    I.t[r] = -(T.R[r] * T.t[0] + T.R[3 + r] * T.t[1] + T.R[6 + r] * T.t[2]);
  }
  return I;
}

// One factor, evaluated by the 64 lanes of one wave (lane = threadIdx.x & 63) through `lds` (120 doubles of this wave's own): every lane derives e and hx^-1 (the
// same operands, the same instructions: the same bits), lanes 0-35 then hold an entry of J_a and of Lambda, and each product entry is ONE lane's sum over m = 0..5 in
// order -- no atomics, no order that depends on the launch.  rec (may be null): the gp_linearized6 record, two of its 122 doubles per lane; err (may be null): the
// factor's error(), the same bits as the record's word 1.  Every lane of the workgroup calls (the barriers are the workgroup's).
__device__ __forceinline__ void pose_factor_eval(const gp_pose_factor& f, const double* __restrict__ poses, double* __restrict__ lds, double* __restrict__ rec,
                                                 double* __restrict__ err) {
  double* sJ = lds;         // J_a (row-major), between only
  double* sL = lds + 36;    // Lambda (row-major: information[] is column-major)
  double* sLJ = lds + 72;   // Lambda J_a
  double* sE = lds + 108;   // e
  double* sLE = lds + 114;  // Lambda e
  const int lane = threadIdx.x & 63;
  const bool between = f.kind == GP_POSE_FACTOR_BETWEEN;
  const Rigid Ta = load_rigid(poses + 16 * (size_t)f.pose_a);
  const Rigid Z = load_rigid(f.measured);
  Rigid hx = Ta;
  if (between) hx = between_rigid(Ta, load_rigid(poses + 16 * (size_t)f.pose_b));
  double e[6];
  pose3_logmap(between_rigid(Z, hx), e);
  // (a lane's entry is SELECTED out of the unrolled set: an array indexed by the lane would live in scratch)
  const Rigid Hi = inverse_rigid(hx);
  double v0 = 0.0;
#pragma unroll
  for (int k = 0; k < 36; k++)
    if (k == lane && between) v0 = -adjoint(Hi, k / 6, k % 6);
#pragma unroll
  for (int k = 0; k < 6; k++)
    if (k + 36 == lane) v0 = e[k];
  if (lane < 36) {
    sJ[lane] = v0;
    sL[lane] = f.information[(lane % 6) * 6 + lane / 6];
  } else if (lane < 42) {
    sE[lane - 36] = v0;
  }
  __syncthreads();
  if (lane < 36) {
    const int r = lane / 6, c = lane % 6;
    double s = 0.0;
    for (int m = 0; m < 6; m++) s += sL[r * 6 + m] * sJ[m * 6 + c];
    sLJ[lane] = s;
  } else if (lane < 42) {
    const int r = lane - 36;
    double s = 0.0;
    for (int m = 0; m < 6; m++) s += sL[r * 6 + m] * sE[m];
    sLE[r] = s;
  }
  __syncthreads();
  double ee = 0.0;
  for (int m = 0; m < 6; m++) ee += sE[m] * sLE[m];
  ee *= 0.5;
  if (err && lane == 0) *err = ee;
  if (!rec) return;
  for (int q = 0; q < 2; q++) {
    const int idx = lane + 64 * q;
    if (idx >= 122) break;
    double v = 0.0;
    if (idx == 1) {
      v = ee;
    } else if (idx >= 2 && idx < 38) {  // H_target = J_a^T Lambda J_a, column-major
      const int r = (idx - 2) % 6, c = (idx - 2) / 6;
      if (between)
        for (int m = 0; m < 6; m++) v += sJ[m * 6 + r] * sLJ[m * 6 + c];
    } else if (idx >= 38 && idx < 74) {  // H_source = J_b^T Lambda J_b = Lambda (J_b = I; a prior's J_a = I)
      const int r = (idx - 38) % 6, c = (idx - 38) / 6;
      v = sL[r * 6 + c];
    } else if (idx >= 74 && idx < 110) {  // H_target_source = J_a^T Lambda J_b = J_a^T Lambda
      const int r = (idx - 74) % 6, c = (idx - 74) / 6;
      if (between)
        for (int m = 0; m < 6; m++) v += sJ[m * 6 + r] * sL[m * 6 + c];
    } else if (idx >= 110 && idx < 116) {  // b_target = J_a^T Lambda e
      const int r = idx - 110;
      if (between)
        for (int m = 0; m < 6; m++) v += sJ[m * 6 + r] * sLE[m];
    } else if (idx >= 116) {  // b_source = Lambda e
      v = sLE[idx - 116];
    }
    rec[idx] = v;  // (idx 0: num_inliers = 0)
  }
}

}  // namespace gp

namespace gp {

// host side (gp_pose_factors.hip), shared with the LM graph (gp_lm.hip)
// the argument checks of gp_pose_factors_create / gp_lm_graph_create_with_pose_factors: GP_ERROR_INVALID_ARGUMENT, named after `api`, or GP_OK
int check_pose_factors(const gp_pose_factor* factors, int num_factors, int num_poses, const char* api);
// factors_dev [num_factors] at poses_dev [N][16] -> records [num_factors] and / or errors [num_factors] (either may be null; host-pinned memory is fine): one launch
int launch_pose_factors(const gp_pose_factor* factors_dev, int num_factors, const double* poses_dev, gp_linearized6* records, double* errors, hipStream_t stream);

}  // namespace gp
