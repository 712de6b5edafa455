// gp_alignment.hpp -- what the registration units (gp_registration.hip: RANSAC and gp_align_points; gp_gnc.hip: graduated non-convexity) share: THE closed forms of
// align_points_se3 / align_points_4dof (registration/alignment.cpp:11-139) -- rotation_from_H3, rotation_from_H2, pose_from_H --, the weighted means and the
// outer-product accumulation of the weighted N-point alignment with its fixed-order tree reduction, the identity pose, and the library's counter-based generator.
// The arithmetic a host restatement reproduces is written without fused multiply-adds: a unit that includes this header switches contraction off first
// (#pragma clang fp contract(off)).
#pragma once

#include <cmath>

#include "gp_host.hpp"

namespace gp {

struct Vec3 {
  double x, y, z;
};
__host__ __device__ __forceinline__ double dot3(const Vec3& a, const Vec3& b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
__host__ __device__ __forceinline__ Vec3 cross3(const Vec3& a, const Vec3& b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
__host__ __device__ __forceinline__ Vec3 scale3(const Vec3& a, double s) { return {a.x * s, a.y * s, a.z * s}; }
__host__ __device__ __forceinline__ Vec3 axpy3(const Vec3& a, double s, const Vec3& b) { return {a.x + s * b.x, a.y + s * b.y, a.z + s * b.z}; }  // a + s b

// one Jacobi rotation of the column pair (ap, aq) of A = H V (and of V): makes the two columns orthogonal
__host__ __device__ __forceinline__ bool jacobi_pair(Vec3& ap, Vec3& aq, Vec3& vp, Vec3& vq) {
  const double alpha = dot3(ap, ap), beta = dot3(aq, aq), gamma = dot3(ap, aq);
  if (!(fabs(gamma) > 1e-15 * sqrt(alpha * beta))) return false;
  const double zeta = (beta - alpha) / (2.0 * gamma);
  const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
  const double c = 1.0 / sqrt(1.0 + t * t), s = c * t;
  const Vec3 a0 = ap, v0 = vp;
  ap = axpy3(scale3(a0, c), -s, aq);
  aq = axpy3(scale3(aq, c), s, a0);
  vp = axpy3(scale3(v0, c), -s, vq);
  vq = axpy3(scale3(vq, c), s, v0);
  return true;
}

__host__ __device__ __forceinline__ void swap_if_less(double& na, double& nb, Vec3& aa, Vec3& ab, Vec3& va, Vec3& vb) {
  if (na < nb) {
    const double n = na;
    na = nb;
    nb = n;
    const Vec3 a = aa;
    aa = ab;
    ab = a;
    const Vec3 v = va;
    va = vb;
    vb = v;
  }
}

// R (row-major r[9]) = U diag(1, 1, det(U) det(V)) V^T of the 3x3 matrix H (row-major h[9], H = sum (t - mt)(s - ms)^T): the columns of A = H V are made
// orthogonal by one-sided Jacobi rotations (V their product), u1, u2 are the two longest columns normalised (u2 re-orthogonalised against u1; any unit vector
// orthogonal to u1 when the column vanishes: a collinear sample), and the third pair is (u1 x u2, v1 x v2), which carries the reference's sign rule.
__host__ __device__ inline void rotation_from_H3(const double* h, double* r) {
  Vec3 a0{h[0], h[3], h[6]}, a1{h[1], h[4], h[7]}, a2{h[2], h[5], h[8]};
  Vec3 v0{1, 0, 0}, v1{0, 1, 0}, v2{0, 0, 1};
  for (int sweep = 0; sweep < 30; sweep++) {
    bool any = jacobi_pair(a0, a1, v0, v1);
    any |= jacobi_pair(a0, a2, v0, v2);
    any |= jacobi_pair(a1, a2, v1, v2);
    if (!any) break;
  }
  double n0 = sqrt(dot3(a0, a0)), n1 = sqrt(dot3(a1, a1)), n2 = sqrt(dot3(a2, a2));
  swap_if_less(n0, n1, a0, a1, v0, v1);
  swap_if_less(n0, n2, a0, a2, v0, v2);
  swap_if_less(n1, n2, a1, a2, v1, v2);
  if (!(n0 > 0.0) || !(n0 < INFINITY)) {  // H = 0 (or not finite): the identity
    for (int i = 0; i < 9; i++) r[i] = i % 4 == 0 ? 1.0 : 0.0;
    return;
  }
  const Vec3 u1 = scale3(a0, 1.0 / n0);
  Vec3 u2 = axpy3(a1, -dot3(u1, a1), u1);
  double m = sqrt(dot3(u2, u2));
  if (!(m > 1e-200)) {  // no second direction: the axis on which u1 is smallest, made orthogonal to u1
    const double ax = fabs(u1.x), ay = fabs(u1.y), az = fabs(u1.z);
    const Vec3 e = (ax <= ay && ax <= az) ? Vec3{1, 0, 0} : (ay <= az ? Vec3{0, 1, 0} : Vec3{0, 0, 1});
    u2 = axpy3(e, -dot3(u1, e), u1);
    m = sqrt(dot3(u2, u2));
  }
  u2 = scale3(u2, 1.0 / m);
  u2 = axpy3(u2, -dot3(u1, u2), u1);
  u2 = scale3(u2, 1.0 / sqrt(dot3(u2, u2)));
  const Vec3 u3 = cross3(u1, u2), w1 = v0, w2 = v1, w3 = cross3(v0, v1);
  r[0] = (u1.x * w1.x + u2.x * w2.x) + u3.x * w3.x;
  r[1] = (u1.x * w1.y + u2.x * w2.y) + u3.x * w3.y;
  r[2] = (u1.x * w1.z + u2.x * w2.z) + u3.x * w3.z;
  r[3] = (u1.y * w1.x + u2.y * w2.x) + u3.y * w3.x;
  r[4] = (u1.y * w1.y + u2.y * w2.y) + u3.y * w3.y;
  r[5] = (u1.y * w1.z + u2.y * w2.z) + u3.y * w3.z;
  r[6] = (u1.z * w1.x + u2.z * w2.x) + u3.z * w3.x;
  r[7] = (u1.z * w1.y + u2.z * w2.y) + u3.z * w3.y;
  r[8] = (u1.z * w1.z + u2.z * w2.z) + u3.z * w3.z;
}

// align_points_4dof's rotation: U diag(1, det(U) det(V)) V^T of H's 2x2 block is the rotation about z that maximises trace(R^T H) = cos (h00 + h11) + sin (h10 - h01)
__host__ __device__ inline void rotation_from_H2(const double* h, double* r) {
  const double c = h[0] + h[4], s = h[3] - h[1];
  const double n = sqrt(c * c + s * s);
  for (int i = 0; i < 9; i++) r[i] = i % 4 == 0 ? 1.0 : 0.0;
  if (!(n > 0.0) || !(n < INFINITY)) return;
  r[0] = c / n;
  r[1] = -(s / n);
  r[3] = s / n;
  r[4] = c / n;
}

// pose (column-major 16) from H and the two means: translation = mean_t - R mean_s (alignment.cpp:37)
__host__ __device__ inline void pose_from_H(const double* h, const Vec3& mt, const Vec3& ms, int dof, double* pose) {
  double r[9];
  if (dof == 6)
    rotation_from_H3(h, r);
  else
    rotation_from_H2(h, r);
  pose[0] = r[0], pose[1] = r[3], pose[2] = r[6], pose[3] = 0.0;
  pose[4] = r[1], pose[5] = r[4], pose[6] = r[7], pose[7] = 0.0;
  pose[8] = r[2], pose[9] = r[5], pose[10] = r[8], pose[11] = 0.0;
  pose[12] = mt.x - ((r[0] * ms.x + r[1] * ms.y) + r[2] * ms.z);
  pose[13] = mt.y - ((r[3] * ms.x + r[4] * ms.y) + r[5] * ms.z);
  pose[14] = mt.z - ((r[6] * ms.x + r[7] * ms.y) + r[8] * ms.z);
  pose[15] = 1.0;
}

__host__ __device__ inline void set_identity16(double* pose) {  // column-major 4x4
  for (int i = 0; i < 16; i++) pose[i] = i % 5 == 0 ? 1.0 : 0.0;
}

__device__ __forceinline__ Vec3 point_f64(const float* __restrict__ p, int i) { return {(double)p[3 * (size_t)i], (double)p[3 * (size_t)i + 1], (double)p[3 * (size_t)i + 2]}; }
__device__ __forceinline__ Vec3 point_f64(const double* __restrict__ p, int i) { return {p[3 * (size_t)i], p[3 * (size_t)i + 1], p[3 * (size_t)i + 2]}; }
__device__ __forceinline__ Vec3 sub3(const Vec3& a, const Vec3& b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
__device__ __forceinline__ double norm3(const Vec3& a) { return sqrt(dot3(a, a)); }
__device__ __forceinline__ void add_outer(double* h, double w, const Vec3& t, const Vec3& s) {
  h[0] += w * t.x * s.x, h[1] += w * t.x * s.y, h[2] += w * t.x * s.z;
  h[3] += w * t.y * s.x, h[4] += w * t.y * s.y, h[5] += w * t.y * s.z;
  h[6] += w * t.z * s.x, h[7] += w * t.z * s.y, h[8] += w * t.z * s.z;
}

// the first pass of a weighted alignment: m[0..6] += w, w t, w s; and the two means from the totals
__device__ __forceinline__ void add_weighted(double* m, double w, const Vec3& t, const Vec3& s) {
  m[0] += w;
  m[1] += w * t.x, m[2] += w * t.y, m[3] += w * t.z;
  m[4] += w * s.x, m[5] += w * s.y, m[6] += w * s.z;
}
struct Means {
  Vec3 t, s;
};
__device__ __forceinline__ Means weighted_means(const double* m) { return {{m[1] / m[0], m[2] / m[0], m[3] / m[0]}, {m[4] / m[0], m[5] / m[0], m[6] / m[0]}}; }

// the tree reduction of the one-workgroup kernels (fixed order, no floating-point atomics): v[count] of every thread -> component k combined over the workgroup by
// op(k, a, b), in every thread; lds holds count x kAlignThreads doubles
constexpr int kAlignThreads = 256;
template <class Op>
__device__ __forceinline__ void block_reduce(double* lds, double* v, int count, Op op) {
  __syncthreads();
  for (int k = 0; k < count; k++) lds[k * kAlignThreads + threadIdx.x] = v[k];
  __syncthreads();
  for (int off = kAlignThreads / 2; off > 0; off >>= 1) {
    if ((int)threadIdx.x < off)
      for (int k = 0; k < count; k++) {
        const double other = lds[k * kAlignThreads + threadIdx.x + off];
        lds[k * kAlignThreads + threadIdx.x] = op(k, lds[k * kAlignThreads + threadIdx.x], other);
      }
    __syncthreads();
  }
  for (int k = 0; k < count; k++) v[k] = lds[k * kAlignThreads];
}
__device__ __forceinline__ void block_sum(double* lds, double* v, int count) { block_reduce(lds, v, count, [](int, double a, double b) { return a + b; }); }

// the library's counter-based generator (include/gtsam_points_hip.h, gp_ransac_estimate_pose): draw `draw` of iteration `iteration`, an index below n
__host__ __device__ __forceinline__ uint64_t ransac_mix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
__host__ __device__ __forceinline__ unsigned ransac_sample_index(uint64_t seed, unsigned iteration, unsigned draw, unsigned n) {
  const uint64_t G = 0x9E3779B97F4A7C15ull;
  const uint64_t r = ransac_mix(ransac_mix(seed + G * ((uint64_t)iteration + 1)) + G * ((uint64_t)draw + 1));
  return (unsigned)(((r >> 32) * (uint64_t)n) >> 32);
}

}  // namespace gp
