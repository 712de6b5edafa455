// gp_eig3.hpp -- the closed-form eigen-decomposition of a symmetric 3 x 3 matrix in f64 (eig3_direct, with eig3_roots and eig3_extract_kernel) and the 3 x 3 inverse
// (inverse3_general).  Device-only maths, no kernels: gp_covariance_point.hpp turns a neighbourhood's sample covariance into V diag(1e-3, 1, 1) V^-1 and the normal
// with it, gp_covariance.hip's normals_from_covs_kernel takes the normal of a given covariance.
//
// Replaces (reference, CPU only): Eigen 3.4.0 SelfAdjointEigenSolver<Matrix3d>::computeDirect and Matrix3d::inverse as features/covariance_estimation.cpp:45-53 and
// features/normal_estimation.cpp:18-55 call them.
#pragma once

#include <type_traits>

#include <hip/hip_runtime.h>

namespace gp {

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
// would get 72 B per lane of LDS for it.  A second copy rather than one shared form, because the covariances are held to the bits they had: with the compile-time
// form everywhere, and also with one generic body that the default calls with run-time ints, the search kernels keep their registers and occupancy (the first
// with less scratch) but the compiler orders and contracts the multiply-adds otherwise, and a few ill-conditioned neighbourhoods -- duplicated points, collinear
// triples at k = 5 -- come out with other last bits, 34 to 39 of 252 output arrays of the tests' clouds.  Whoever merges the two re-baselines those.
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

}  // namespace gp
