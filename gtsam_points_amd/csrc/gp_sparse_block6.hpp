// gp_sparse_block6.hpp -- the 6 x 6 pieces of the block-sparse LL^T that every numeric kernel shares (gp_sparse_multi.hpp, gp_sparse_small.hip)
#pragma once
#include "gp_damped_step.hpp"

namespace gp {

// visibility of LDS writes between the lanes of ONE wave (its LDS operations execute in program order; this keeps the compiler from
// moving them and makes it wait for the writes): what __syncthreads() is for a workgroup, without the s_barrier
#define GP_WAVE_SYNC_LDS()                                   \
  do {                                                       \
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");   \
    __builtin_amdgcn_wave_barrier();                         \
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");   \
  } while (0)

// ---- the 6 x 6 pieces every numeric kernel shares (round 6) ------------------------------------------------------------------------------------------------------------
// A column of the factorisation is ONE dependent chain -- gather -> 6 x 6 Cholesky -> forward substitution / the blocks below -- and rounds 1-5 spent it on IEEE f64
// divisions and square roots (18 divisions + 6 square roots per column on the chain, ~300 clocks each) and on LDS round trips between them: 6-8 us per column whether
// the operands sat in L2 or in LDS (profiles/r06_solver_step_time_one.jsonl).  Now a pivot costs one reciprocal square root (hardware estimate + two Newton steps, ~1 ulp)
// and everything that divided by a diagonal entry multiplies by the stored reciprocal; the substitutions run out of registers.  All four kernels call THESE functions, so
// the one-launch step and the multi-launch form stay bit-identical by construction.
__device__ __forceinline__ double rsqrt_f64(double x) {  // x > 0
  double y = __builtin_amdgcn_rsq(x);
  const double hx = 0.5 * x;
#pragma unroll
  for (int it = 0; it < 2; it++) {  // y <- y + y (1/2 - (x / 2) y^2)
    const double e = __builtin_fma(-(hx * y), y, 0.5);
    y = __builtin_fma(y, e, y);
  }
  return y;
}
// ONE wave, all 64 lanes call (lane j < 36 = entry (r, c) = (j % 6, j / 6)): the lower triangle of D (LDS, row stride 7) becomes its Cholesky factor, dinv[p] = 1 / L_pp.
// A pivot that is not positive raises *bad and is replaced by 1 (the caller reports an indeterminate system).
// The entries live in the lanes' registers between the one read and the one write of D: a pivot is broadcast with v_readlane, the two column entries an update needs come
// through ds_bpermute -- no LDS round trip + wait per step (the LDS form measured 480 clocks per pivot: scripts/r06/solver_trace.py).
__device__ __forceinline__ double lane_bcast_f64(double v, const int src_lane /* compile-time constant after unrolling */) {
  const unsigned long long b = __builtin_bit_cast(unsigned long long, v);
  const unsigned lo = __builtin_amdgcn_readlane((int)(unsigned)b, src_lane), hi = __builtin_amdgcn_readlane((int)(unsigned)(b >> 32), src_lane);
  return __builtin_bit_cast(double, ((unsigned long long)hi << 32) | (unsigned long long)lo);
}
// A pivot is held against the column's six assembled diagonal entries (scale6): pivot_ok.
__device__ __forceinline__ void chol6_wave(double (*D)[7], double* dinv, const int j, int* bad, const double* scale6) {
  const int r = j % 6, c = j / 6;
  double a = j < 36 ? D[r][c] : 0.0;
  double dv[6], sc[6];
#pragma unroll
  for (int p = 0; p < 6; p++) sc[p] = scale6[p];
  bool any_bad = false;
#pragma unroll
  for (int p = 0; p < 6; p++) {
    double piv = lane_bcast_f64(a, 7 * p);  // D[p][p]: wave-uniform
    if (!pivot_ok(piv, sc[p])) {
      any_bad = true;
      piv = 1.0;
    }
    const double rl = rsqrt_f64(piv);
    const double l = piv * rl;
    dv[p] = rl;
    if (j < 36 && c == p && r >= p) a = r == p ? l : a * rl;
    // the column just scaled: entry (r, p) for the lane's row, entry (c, p) for its column (every lane asks: the shuffles are wave-wide)
    const double arp = __shfl(a, (r + 6 * p) & 63, 64), acp = __shfl(a, (c + 6 * p) & 63, 64);
    if (j < 36 && c > p && r >= c) a = __builtin_fma(-arp, acp, a);
  }
  if (j < 36) D[r][c] = a;
  if (j == 36) {
#pragma unroll
    for (int p = 0; p < 6; p++) dinv[p] = dv[p];
  }
  if (j == 0 && any_bad) *bad = 1;
  GP_WAVE_SYNC_LDS();
}
// ONE lane: rhs <- L^-1 rhs by forward substitution, out of registers (every operand is requested before the chain starts)
__device__ __forceinline__ void forward6(double (*D)[7], const double* dinv, double* rhs) {
  double d[6][6], iv[6], y[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    iv[i] = dinv[i];
    y[i] = rhs[i];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q < i) d[i][q] = D[i][q];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) {
    double sum = y[i];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q < i) sum = __builtin_fma(-d[i][q], y[q], sum);
    y[i] = sum * iv[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) rhs[i] = y[i];
}
// ONE lane: row r of a block below the diagonal, B <- B L^-T (forward substitution along the row); Bk = the block, column-major
// (RM: the block is stored row-major -- the one-launch step's LDS copy -- instead of column-major: same operands, same operations)
template <bool RM = false>
__device__ __forceinline__ void trsm_row6(double* Bk, const int r, double (*D)[7], const double* dinv) {
  double d[6][6], iv[6], o[6];
#pragma unroll
  for (int c = 0; c < 6; c++) {
    iv[c] = dinv[c];
    o[c] = RM ? Bk[6 * r + c] : Bk[r + 6 * c];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q < c) d[c][q] = D[c][q];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) {
    double sum = o[c];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q < c) sum = __builtin_fma(-o[q], d[c][q], sum);
    o[c] = sum * iv[c];
  }
#pragma unroll
  for (int c = 0; c < 6; c++) (RM ? Bk[6 * r + c] : Bk[r + 6 * c]) = o[c];
}
// ONE lane: x_k = L_kk^-T v by backward substitution; Dk = the factored diagonal block, column-major; dinv_k = the reciprocals of its diagonal
template <bool RM = false>
__device__ __forceinline__ void back6(const double* Dk, const double* dinv_k, const double* v, double* xk_out) {
  double d[6][6], iv[6], xk[6];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    iv[i] = dinv_k[i];
    xk[i] = v[i];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q > i) d[q][i] = RM ? Dk[6 * q + i] : Dk[q + 6 * i];  // (L^T)_{iq} = L_{qi}
  }
#pragma unroll
  for (int i = 5; i >= 0; i--) {
    double sum = xk[i];
#pragma unroll
    for (int q = 0; q < 6; q++)
      if (q > i) sum = __builtin_fma(-d[q][i], xk[q], sum);
    xk[i] = sum * iv[i];
  }
#pragma unroll
  for (int i = 0; i < 6; i++) xk_out[i] = xk[i];
}

// a row of a ROW-major block in LDS (the one-launch step's copy): 48 contiguous, 16-byte-aligned bytes = three 128-bit accesses instead of six 64-bit ones
__device__ __forceinline__ void load_row6(const double* row, double* a) {
  const double2* A = reinterpret_cast<const double2*>(row);
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const double2 x = A[q];
    a[2 * q] = x.x, a[2 * q + 1] = x.y;
  }
}
__device__ __forceinline__ void store_row6(double* row, const double* a) {
  double2* O = reinterpret_cast<double2*>(row);
#pragma unroll
  for (int q = 0; q < 3; q++) O[q] = make_double2(a[2 * q], a[2 * q + 1]);
}

}  // namespace gp
