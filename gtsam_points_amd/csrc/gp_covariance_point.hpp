// gp_covariance_point.hpp -- what the covariance and normal estimator stores for ONE point: the identity for a point without k neighbours (store_identity), the
// normal after the sign rule (store_normal), and the regularised covariance V diag(1e-3, 1, 1) V^-1 of a neighbour list with the normal beside it
// (covariance_from_neighbours).  Device code only, no kernels: the kernels of gp_covariance.hip, gp_covariance_far.hpp and gp_covariance_rows.hpp call it.
//
// Replaces (reference, CPU only): features/covariance_estimation.cpp:27-53, features/normal_estimation.cpp:18-55.
#pragma once

#include "gp_eig3.hpp"
#include "gp_knn_search.hpp"

namespace gp {

// non-finite points have no neighbours: identity covariance, counted as "short" (covariance_estimation.cpp:27-31)
// NORMALS (estimate_normals, features/normal_estimation.cpp:18-50): the identity's eigenbasis is the identity (computeDirect's triple root), so the normal is
// (1, 0, 0), turned round when p . n = p.x > 1 (:26).  covs may be null then (the normals-only call).
template <bool NORMALS>
__device__ __forceinline__ void store_identity(float qx, float* __restrict__ cov_out, float* __restrict__ normal_out) {
  if constexpr (NORMALS) {
    normal_out[0] = qx > 1.0f ? -1.0f : 1.0f;
    normal_out[1] = 0.0f;
    normal_out[2] = 0.0f;
    if (!cov_out) return;
  }
  for (int j = 0; j < 9; j++) cov_out[j] = (j % 4 == 0) ? 1.0f : 0.0f;
}

// estimate_covariances (features/covariance_estimation.cpp:18-77): k-NN (query included) -> sample covariance ->
// V diag(1e-3, 1, 1) V^-1.  Fewer than k neighbours -> identity (:27-31).
// sample covariance of the k neighbours -> V diag(1e-3, 1, 1) V^-1 (features/covariance_estimation.cpp:33-53)
// NORMALS: the first eigenvector IS estimate_normals(points, n, k)'s normal (features/normal_estimation.cpp:52-55: the eigenvector of the smallest eigenvalue of
// V diag(1e-3, 1, 1) V^-1 is V's first column), stored beside the covariance, or instead of it when out == nullptr (then no inverse and no V L V^-1 products)
__device__ __forceinline__ void store_normal(const double* v, double qx, double qy, double qz, float* __restrict__ normal_out) {
  const bool away = qx * v[0] + qy * v[1] + qz * v[2] > 1.0;  // :26, points in the sensor frame
  normal_out[0] = (float)(away ? -v[0] : v[0]);
  normal_out[1] = (float)(away ? -v[1] : v[1]);
  normal_out[2] = (float)(away ? -v[2] : v[2]);
}

template <int KMAX, bool FULL, bool NORMALS = false>
__device__ __forceinline__ void covariance_from_neighbours(const TopK<KMAX, FULL>& top, const float* __restrict__ points, int k, float* __restrict__ out,
                                                           float* __restrict__ normal_out = nullptr, double qx = 0.0, double qy = 0.0, double qz = 0.0) {
  double sp[3] = {0, 0, 0}, spp[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
  for (int j = 0; j < KMAX; j++)
    if (j < k) {
      const size_t nb = (size_t)top.idx[j];
      const double p[3] = {(double)points[3 * nb], (double)points[3 * nb + 1], (double)points[3 * nb + 2]};
      for (int r = 0; r < 3; r++) sp[r] += p[r];
      for (int c = 0; c < 3; c++)
        for (int r = 0; r < 3; r++) spp[c * 3 + r] += p[r] * p[c];
    }
  double cov[9];
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) cov[c * 3 + r] = (spp[c * 3 + r] - (sp[r] / (double)k) * sp[c]) / (double)k;  // :43
  double evals[3], V[9], Vinv[9];
  eig3_direct(cov, evals, V);
  if constexpr (NORMALS) {
    store_normal(V, qx, qy, qz, normal_out);
    if (!out) return;
  }
  inverse3_general(V, Vinv);
  const double lam[3] = {1e-3, 1.0, 1.0};
  for (int c = 0; c < 3; c++)
    for (int r = 0; r < 3; r++) {
      double s = 0.0;
      for (int kk = 0; kk < 3; kk++) s += V[kk * 3 + r] * lam[kk] * Vinv[c * 3 + kk];
      out[c * 3 + r] = (float)s;
    }
}

}  // namespace gp
