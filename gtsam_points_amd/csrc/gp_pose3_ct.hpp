// gp_pose3_ct.hpp -- the Pose3 pieces of the continuous-time factors (gp_ct_factors.hip) beside those of gp_pose_factors.hpp: the SE(3) exponential and logarithm
// with series coefficients, gtsam::Pose3::ExpmapDerivative / LogmapDerivative (the right Jacobian Jr and its inverse, tangent (omega, v)), and one entry of the
// factor's pose table with its two derivative blocks.  f64 throughout.
//
// Every coefficient that is a difference of nearly equal terms at a small angle -- (1 - cos)/th^2, (th - sin)/th^3, ... -- is summed as its power series below
// theta = 1/2 and evaluated in closed form above, where the cancellation costs two digits at most.  T0 == T1 (theta = 0) is where every odometry iteration starts.
#pragma once
#include "gp_pose_factors.hpp"

namespace gp {

constexpr double inv_factorial(int n) {
  double f = 1.0;
  for (int i = 2; i <= n; i++) f *= (double)i;
  return 1.0 / f;
}

// sum over k < N of (-x)^k / (2 k + M)!, Horner from the tail
template <int M, int N>
__device__ __forceinline__ double alternating_series(double x) {
  double s = 0.0;
#pragma unroll
  for (int k = N - 1; k >= 0; k--) s = inv_factorial(2 * k + M) - x * s;
  return s;
}

// A = sin th / th, B = (1 - cos th) / th^2, C = (th - sin th) / th^3, D = (1 - th^2 / 2 - cos th) / th^4, E = (th - sin th - th^3 / 6) / th^5
struct So3Coeffs {
  double A, B, C, D, E;
};
constexpr double kSeriesTheta2 = 0.25;  // series below theta = 1/2: nine terms leave less than 1e-20

__device__ __forceinline__ So3Coeffs so3_coeffs(double th2) {
  So3Coeffs k;
  if (th2 < kSeriesTheta2) {
    k.A = alternating_series<1, 9>(th2);
    k.B = alternating_series<2, 9>(th2);
    k.C = alternating_series<3, 9>(th2);
    k.D = -alternating_series<4, 9>(th2);
    k.E = -alternating_series<5, 9>(th2);
  } else {
    const double th = sqrt(th2), s = sin(th), c = cos(th);
    k.A = s / th;
    k.B = (1.0 - c) / th2;
    k.C = (th - s) / (th2 * th);
    k.D = (1.0 - 0.5 * th2 - c) / (th2 * th2);
    k.E = (th - s - th2 * th / 6.0) / (th2 * th2 * th);
  }
  return k;
}

// F = 1 / th^2 - (1 + cos th) / (2 th sin th) = (1 - (th / 2) cot(th / 2)) / th^2 = sum |B_2k| th^(2k-2) / (2k)!: the W^2 coefficient of the SO(3) logarithm's
// derivative and of the translation part of the SE(3) logarithm
__device__ __forceinline__ double so3_log_coeff(double th2) {
  if (th2 < kSeriesTheta2) {
    const double c[9] = {1.0 / 12.0,
                         1.0 / 720.0,
                         1.0 / 30240.0,
                         1.0 / 1209600.0,
                         1.0 / 47900160.0,
                         691.0 / 1307674368000.0,
                         1.0 / 74724249600.0,
                         3617.0 / 10670622842880000.0,
                         43867.0 / 5109094217170944000.0};
    double s = 0.0;
#pragma unroll
    for (int k = 8; k >= 0; k--) s = c[k] + th2 * s;
    return s;
  }
  const double th = sqrt(th2);
  return 1.0 / th2 - (1.0 + cos(th)) / (2.0 * th * sin(th));
}

// 3x3 helpers, row-major
__device__ __forceinline__ void skew3(const double* __restrict__ w, double* __restrict__ W) {
  W[0] = 0.0, W[1] = -w[2], W[2] = w[1];
  W[3] = w[2], W[4] = 0.0, W[5] = -w[0];
  W[6] = -w[1], W[7] = w[0], W[8] = 0.0;
}
__device__ __forceinline__ void mul3(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C) {
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) C[r * 3 + c] = A[r * 3] * B[c] + A[r * 3 + 1] * B[3 + c] + A[r * 3 + 2] * B[6 + c];
}

// gtsam::Pose3::Expmap(xi), xi = (omega, v): R = I + A W + B W^2, t = (I + B W + C W^2) v
__device__ __forceinline__ Rigid pose3_expmap(const double* __restrict__ xi, const So3Coeffs& k) {
  double W[9], W2[9];
  skew3(xi, W);
  mul3(W, W, W2);
  Rigid X;
  double V[9];
#pragma unroll
  for (int i = 0; i < 9; i++) {
    const double id = (i % 4 == 0) ? 1.0 : 0.0;
    X.R[i] = id + k.A * W[i] + k.B * W2[i];
    V[i] = id + k.B * W[i] + k.C * W2[i];
  }
#pragma unroll
  for (int r = 0; r < 3; r++) X.t[r] = V[r * 3] * xi[3] + V[r * 3 + 1] * xi[4] + V[r * 3 + 2] * xi[5];
  return X;
}

// T X
__device__ __forceinline__ Rigid compose_rigid(const Rigid& T, const Rigid& X) {
  Rigid out;
  mul3(T.R, X.R, out.R);
#pragma unroll
  for (int r = 0; r < 3; r++) out.t[r] = T.R[r * 3] * X.t[0] + T.R[r * 3 + 1] * X.t[1] + T.R[r * 3 + 2] * X.t[2] + T.t[r];
  return out;
}

// gtsam::Pose3::Logmap: omega from so3_logmap, v = (I - W / 2 + F W^2) t (pose3_logmap's own formula with its W^2 coefficient (1 - th / (2 tan(th / 2))) / th^2 = F
// as a series at small angles)
__device__ __forceinline__ void pose3_logmap_series(const Rigid& T, double* __restrict__ xi) {
  double w[3];
  so3_logmap(T.R, w);
  const double F = so3_log_coeff(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
  const double wt[3] = {w[1] * T.t[2] - w[2] * T.t[1], w[2] * T.t[0] - w[0] * T.t[2], w[0] * T.t[1] - w[1] * T.t[0]};
  const double wwt[3] = {w[1] * wt[2] - w[2] * wt[1], w[2] * wt[0] - w[0] * wt[2], w[0] * wt[1] - w[1] * wt[0]};
#pragma unroll
  for (int i = 0; i < 3; i++) {
    xi[i] = w[i];
    xi[3 + i] = T.t[i] - 0.5 * wt[i] + F * wwt[i];
  }
}

// gtsam::Pose3::ComputeQforExpmapDerivative (Barfoot, eq. 102 with the signs of the right Jacobian):
//   Q = -V / 2 + C (W V + V W - W V W) + D (W^2 V + V W^2 - 3 W V W) - (D - 3 E) / 2 (W V W^2 + W^2 V W)
__device__ __forceinline__ void pose3_q(const double* __restrict__ xi, const So3Coeffs& k, double* __restrict__ Q) {
  double W[9], V[9], WV[9], VW[9], WVW[9], WW[9], WWV[9], VWW[9], WVWW[9], WWVW[9];
  skew3(xi, W);
  skew3(xi + 3, V);
  mul3(W, V, WV);
  mul3(V, W, VW);
  mul3(WV, W, WVW);
  mul3(W, W, WW);
  mul3(WW, V, WWV);
  mul3(V, WW, VWW);
  mul3(WVW, W, WVWW);
  mul3(W, WVW, WWVW);
  const double h = -0.5 * (k.D - 3.0 * k.E);
#pragma unroll
  for (int i = 0; i < 9; i++) Q[i] = -0.5 * V[i] + k.C * (WV[i] + VW[i] - WVW[i]) + k.D * (WWV[i] + VWW[i] - 3.0 * WVW[i]) + h * (WVWW[i] + WWVW[i]);
}

// gtsam::Pose3::ExpmapDerivative(xi) = [[Jw, 0], [Q, Jw]], Jw = I - B W + C W^2 (gtsam::SO3's right Jacobian); row-major 6x6
__device__ __forceinline__ void pose3_jr(const double* __restrict__ xi, const So3Coeffs& k, double* __restrict__ J) {
  double W[9], W2[9], Q[9];
  skew3(xi, W);
  mul3(W, W, W2);
  pose3_q(xi, k, Q);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      const double jw = (r == c ? 1.0 : 0.0) - k.B * W[r * 3 + c] + k.C * W2[r * 3 + c];
      J[r * 6 + c] = jw;
      J[r * 6 + 3 + c] = 0.0;
      J[(3 + r) * 6 + c] = Q[r * 3 + c];
      J[(3 + r) * 6 + 3 + c] = jw;
    }
}

// gtsam::Pose3::LogmapDerivative at the pose whose logarithm is xi = [[Ji, 0], [-Ji Q Ji, Ji]], Ji = I + W / 2 + F W^2; row-major 6x6
__device__ __forceinline__ void pose3_jr_inv(const double* __restrict__ xi, const So3Coeffs& k, double* __restrict__ J) {
  double W[9], W2[9], Q[9], Ji[9], QJ[9], JQJ[9];
  skew3(xi, W);
  mul3(W, W, W2);
  pose3_q(xi, k, Q);
  const double F = so3_log_coeff(xi[0] * xi[0] + xi[1] * xi[1] + xi[2] * xi[2]);
#pragma unroll
  for (int i = 0; i < 9; i++) Ji[i] = ((i % 4 == 0) ? 1.0 : 0.0) + 0.5 * W[i] + F * W2[i];
  mul3(Q, Ji, QJ);
  mul3(Ji, QJ, JQJ);
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      J[r * 6 + c] = Ji[r * 3 + c];
      J[r * 6 + 3 + c] = 0.0;
      J[(3 + r) * 6 + c] = -JQJ[r * 3 + c];
      J[(3 + r) * 6 + 3 + c] = Ji[r * 3 + c];
    }
}

// AdjointMap(T^-1), row-major 6x6
__device__ __forceinline__ void adjoint_of_inverse(const Rigid& T, double* __restrict__ A) {
  const Rigid I = inverse_rigid(T);
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) A[r * 6 + c] = adjoint(I, r, c);
}

__device__ __forceinline__ void mul6(const double* __restrict__ A, const double* __restrict__ B, double* __restrict__ C) {
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int c = 0; c < 6; c++) {
      double s = 0.0;
#pragma unroll
      for (int m = 0; m < 6; m++) s += A[r * 6 + m] * B[m * 6 + c];
      C[r * 6 + c] = s;
    }
}

constexpr int kCtPoseRow = 12 + 36 + 36;  // doubles per pose-table entry: T(t) 3x4 row-major | D0(t) row-major | D1(t) row-major

// IntegratedCT_ICPFactor_::update_poses (integrated_ct_icp_factor_impl.hpp:202-248) for one table entry t in [0, 1]:
//   delta = T0^-1 T1, vel = Log(delta), inc = Exp(t vel), T(t) = T0 inc,
//   G = t Jr(t vel) Jr^-1(vel)                (H_pose_inc = I, H_inc_vel = Jr(t vel), H_vel_delta = Jr^-1(vel))
//   D0 = Ad(inc^-1) - G Ad(delta^-1)          (H_pose_0_a = Ad(inc^-1), H_delta_0 = -Ad(delta^-1))
//   D1 = G                                    (H_delta_1 = I)
// row: kCtPoseRow doubles; with derivs == false only T(t) is written.
__device__ __forceinline__ void ct_pose_entry(const Rigid& T0, const Rigid& T1, double t, bool derivs, double* __restrict__ row) {
  const Rigid delta = between_rigid(T0, T1);
  double vel[6], xt[6];
  pose3_logmap_series(delta, vel);
#pragma unroll
  for (int i = 0; i < 6; i++) xt[i] = t * vel[i];
  const double th2 = vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2];
  const So3Coeffs kt = so3_coeffs(t * t * th2);
  const Rigid inc = pose3_expmap(xt, kt);
  const Rigid T = compose_rigid(T0, inc);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) row[r * 4 + c] = T.R[r * 3 + c];
    row[r * 4 + 3] = T.t[r];
  }
  if (!derivs) return;
  const So3Coeffs k1 = so3_coeffs(th2);
  double Jt[36], Ji[36], G[36], Ad[36], GA[36];
  pose3_jr(xt, kt, Jt);
  pose3_jr_inv(vel, k1, Ji);
  mul6(Jt, Ji, G);
#pragma unroll
  for (int i = 0; i < 36; i++) G[i] *= t;
  adjoint_of_inverse(delta, Ad);
  mul6(G, Ad, GA);
  adjoint_of_inverse(inc, Ad);
#pragma unroll
  for (int i = 0; i < 36; i++) {
    row[12 + i] = Ad[i] - GA[i];
    row[48 + i] = G[i];
  }
}

}  // namespace gp
