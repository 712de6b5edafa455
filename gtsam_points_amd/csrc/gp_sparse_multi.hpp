// gp_sparse_multi.hpp -- the multi-launch numeric phase of the block-sparse LL^T (gp_sparse.hip): assembly and damping, one factorisation launch and one
// backward-substitution launch per level of the schedule, x back into slot order
#pragma once
#include "gp_damped_step.hpp"
#include "gp_sparse_block6.hpp"

namespace gp {

struct SparseDest {
  int block;         // destination block of L
  int diag_col;      // >= 0: the block is the diagonal block of this column (b is assembled with it)
  int begin, count;  // range in the contribution list
};

// what gp_sparse_system_step folds into the assembly (one launch for: assemble, damp, b and c handed to the host, the status word cleared)
struct SparseStepExtras {
  double lambda, min_diag, max_diag;
  int diagonal;
  const double* prior_diag;  // elimination order, may be null
  const int* perm;           // elimination order -> slot
  double* b_slots_host;      // pinned: b in slot order
  double* c_dev;
  double* c_host;            // pinned
  int* status;
  int num_factors, num_dests;
  double* diag0;             // [6 P], elimination order: the assembled (damped) diagonal of A, the scale a pivot is held against (kPivotTolerance)
};

// A's blocks into their places in L's storage (every block of L has a destination: fill blocks have an empty contribution list and become zero) + b, one 64-lane
// workgroup per destination, factor order.  STEP: the damping of sparse_damp_kernel applied to the diagonal as it is written (damped_diagonal in both), b also stored in
// slot order where the host reads it, and one extra workgroup that sums the errors (sum_errors, as sum_errors_kernel) and clears the status
template <bool STEP>
__global__ void __launch_bounds__(64) sparse_assemble_kernel(const SparseDest* __restrict__ dests, const Contribution* __restrict__ contribs,
                                                             const double* __restrict__ records, double* __restrict__ L, double* __restrict__ b, const SparseStepExtras ex) {
  const int t = threadIdx.x;
  if (STEP && (int)blockIdx.x == ex.num_dests) {
    const double c = sum_errors<64>(records, ex.num_factors);
    if (t == 0) {
      *ex.c_dev = c;
      *ex.c_host = c;
      *ex.status = 0;
    }
    return;
  }
  const SparseDest d = dests[blockIdx.x];
  if (t < 36) {
    const int r = t % 6, c = t / 6;
    double s = gather_h(contribs, d.begin, d.count, records, r, c);
    if (STEP && d.diag_col >= 0 && r == c && (ex.lambda > 0.0 || ex.prior_diag))
      s = damped_diagonal(s, ex.lambda, ex.diagonal, ex.min_diag, ex.max_diag, ex.prior_diag ? ex.prior_diag + 6 * (size_t)d.diag_col + r : nullptr);
    L[36 * (size_t)d.block + t] = s;
    if (d.diag_col >= 0 && r == c) ex.diag0[6 * (size_t)d.diag_col + r] = s;
  } else if (t < 42 && d.diag_col >= 0) {
    const int r = t - 36;
    const double s = gather_g(contribs, d.begin, d.count, records, r);
    b[6 * (size_t)d.diag_col + r] = s;
    if (STEP) ex.b_slots_host[6 * (size_t)ex.perm[d.diag_col] + r] = s;
  }
}

__global__ void __launch_bounds__(256) sparse_damp_kernel(double* __restrict__ L, const int* __restrict__ colptr, int n, double lambda, int diagonal, double min_diag,
                                                          double max_diag, const double* __restrict__ prior_diag /*elimination order*/, double* __restrict__ diag0) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  double* p = L + 36 * (size_t)colptr[i / 6] + 7 * (i % 6);
  *p = damped_diagonal(*p, lambda, diagonal, min_diag, max_diag, prior_diag ? prior_diag + i : nullptr);
  diag0[i] = *p;
}

struct SparseView {
  const int* colptr;
  const int* rowidx;
  const int* upd_ptr;
  const int* upd_a;
  const int* upd_b;
  const int* upd_bpos;
  const int* row_ptr;
  const int* row_blk;
  const int* row_col;
  const int* work_ptr;
  const int* work_cols;
  double* L;      // [nnzL][36], column-major 6x6 blocks
  double* y;      // [6 P] forward-substituted right-hand side (in: b), elimination order
  double* x;      // [6 P] solution, elimination order
  double* dinv;   // [6 P] reciprocals of L's diagonal, written with every factored column (the substitutions multiply by them)
  const double* diag0;  // [6 P] the assembled diagonal of A (what a pivot is compared with)
  int* status;    // != 0: a pivot was not positive
};

// what both factor kernels do with a column k (nb blocks from `base`) once it is gathered -- D, rhs, dinv, bad: the workgroup's LDS; all THREADS threads call
template <int THREADS>
__device__ __forceinline__ void sparse_column_tail(const SparseView& S, const int k, const int base, const int nb, const int t, double (*D)[7], double* rhs, double* dinv, int* bad) {
  // 2. the diagonal block: 6x6 Cholesky by the first wave (chol6_wave), then y_k = L_kk^-1 rhs by one lane out of registers
  if (t < 64) {
    chol6_wave(D, dinv, t, bad, S.diag0 + 6 * (size_t)k);
    if (t == 0) forward6(D, dinv, rhs);
  }
  __syncthreads();
  if (t < 36) S.L[36 * (size_t)base + t] = (t % 6) >= (t / 6) ? D[t % 6][t / 6] : 0.0;
  if (t >= 64 && t < 70) S.y[6 * (size_t)k + (t - 64)] = rhs[t - 64];
  if (t >= 70 && t < 76) S.dinv[6 * (size_t)k + (t - 70)] = dinv[t - 70];
  // 3. the blocks below: L_ik = B_ik L_kk^-T, one lane per (block, row): forward substitution along the row (trsm_row6)
  for (int e = t; e < 6 * (nb - 1); e += THREADS) trsm_row6(S.L + 36 * (size_t)(base + 1 + e / 6), e % 6, D, dinv);
  __syncthreads();  // the next column of this list reads these blocks (same compute unit: global writes are visible after the barrier)
}

// left-looking block Cholesky of the columns of work list (first_list + blockIdx.x), in elimination order
template <int THREADS>
__global__ void __launch_bounds__(THREADS) sparse_factor_kernel(SparseView S, int first_list) {
  __shared__ double D[6][7];   // diagonal block (row stride 7: the column sweeps below are conflict-free), becomes L_kk
  __shared__ double rhs[6], dinv[6];
  __shared__ int bad;
  const int list = first_list + blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) bad = 0;
  for (int w = S.work_ptr[list]; w < S.work_ptr[list + 1]; w++) {
    const int k = S.work_cols[w];
    const int base = S.colptr[k], nb = S.colptr[k + 1] - base;
    // 1. gather: every entry of every block of the column collects its updates (ascending source column)
    for (int e = t; e < 36 * nb; e += THREADS) {
      const int d = base + e / 36, r = (e % 36) % 6, c = (e % 36) / 6;
      double acc = S.L[36 * (size_t)d + (e % 36)];
      // the products of an entry are a chain of dependent round trips (index -> block -> value) when taken one at a time: the separator columns of a
      // band graph carry ~100 products per block and took ~27 us apiece.  Four products' indices, then their 48 operands, are requested together;
      // the subtractions keep the order of the list (ascending source column), so the factor is bit for bit what the one-at-a-time loop gives
      int u = S.upd_ptr[d];
      const int ue = S.upd_ptr[d + 1];
      constexpr int kBatch = 4;
      for (; u < ue; u += kBatch) {
        int ia[kBatch], ib[kBatch];
#pragma unroll
        for (int w = 0; w < kBatch; w++) {
          const int uu = u + w < ue ? u + w : ue - 1;  // (a short tail repeats the last product's operands and skips its subtraction)
          ia[w] = S.upd_a[uu];
          ib[w] = S.upd_b[uu];
        }
        double av[kBatch][6], bv[kBatch][6];
#pragma unroll
        for (int w = 0; w < kBatch; w++) {
          const double* A = S.L + 36 * (size_t)ia[w];
          const double* B = S.L + 36 * (size_t)ib[w];
#pragma unroll
          for (int q = 0; q < 6; q++) {
            av[w][q] = A[r + 6 * q];
            bv[w][q] = B[c + 6 * q];
          }
        }
#pragma unroll
        for (int w = 0; w < kBatch; w++)
          if (u + w < ue) {
#pragma unroll
            for (int q = 0; q < 6; q++) acc -= av[w][q] * bv[w][q];
          }
      }
      if (d == base) {
        D[r][c] = acc;
      } else {
        S.L[36 * (size_t)d + (e % 36)] = acc;
      }
    }
    // right-hand side of the forward substitution: b_k - sum_j L_kj y_j
    if (t >= 64 && t < 70) {
      const int r = t - 64;
      double acc = S.y[6 * (size_t)k + r];
      int u = S.row_ptr[k];
      const int ue = S.row_ptr[k + 1];
      for (; u + 4 <= ue; u += 4) {  // four blocks of the row requested together, subtracted in list order (see the gather above)
        int ib[4], ic[4];
#pragma unroll
        for (int w = 0; w < 4; w++) {
          ib[w] = S.row_blk[u + w];
          ic[w] = S.row_col[u + w];
        }
        double av[4][6], yv[4][6];
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
          for (int q = 0; q < 6; q++) {
            av[w][q] = S.L[36 * (size_t)ib[w] + r + 6 * q];
            yv[w][q] = S.y[6 * (size_t)ic[w] + q];
          }
#pragma unroll
        for (int w = 0; w < 4; w++)
#pragma unroll
          for (int q = 0; q < 6; q++) acc -= av[w][q] * yv[w][q];
      }
      for (; u < ue; u++) {
        const double* A = S.L + 36 * (size_t)S.row_blk[u];
        const double* yj = S.y + 6 * (size_t)S.row_col[u];
#pragma unroll
        for (int q = 0; q < 6; q++) acc -= A[r + 6 * q] * yj[q];
      }
      rhs[r] = acc;
    }
    __syncthreads();
    sparse_column_tail<THREADS>(S, k, base, nb, t, D, rhs, dinv, &bad);
  }
  if (t == 0 && bad) atomicOr(S.status, 1);
}

// The same for the chains of SEPARATOR columns (levels > 0): columns of 40-70 blocks whose entries each collect ~100 block products.  In the kernel above
// every entry of a block walks its product list by itself -- 12 loads per product and entry (a 6-row of A, a 6-row of B), four products per dependent round
// trip -- and a 512-pose band graph spent ~20 us per such column, 60 columns one after the other (profiles/r03_solver_time.txt).  Here:
//   * the B operands of a column k are the blocks L_kj of ROW k, the same for every block of the column: they are staged once in LDS (with y_j for the forward
//     substitution), and a product names its B by position in that row (upd_bpos);
//   * one thread owns a ROW of a block (six entries): 6 global loads per product instead of 72 per block-entry set, 36 fma against LDS operands;
//   * the product list of a block row is cut into G contiguous slices (G = what fits the workgroup, <= 8), whose partial sums meet in LDS in slice order:
//     a row's chain of dependent round trips is 1 / G as long.  Fixed order => bit-reproducible; the rounding differs from the one-at-a-time order of the kernel
//     above at the 1e-16 level.
// Columns whose row list exceeds kStageBlocks take the per-entry gather of the kernel above (same results as there).
constexpr int kStageBlocks = 128;
template <int THREADS>
__global__ void __launch_bounds__(THREADS) sparse_factor_staged_kernel(SparseView S, int first_list) {
  __shared__ double Bs[kStageBlocks][36];  // L_kj, j = row list of the column being factored
  __shared__ double ys[kStageBlocks][6];   // y_j
  __shared__ double part[THREADS][6];      // slice partials: [row item * G + slice][c]
  __shared__ double rpart[16][6];
  __shared__ double D[6][7];
  __shared__ double rhs[6], dinv[6];
  __shared__ int bad;
  const int list = first_list + blockIdx.x;
  const int t = threadIdx.x;
  if (t == 0) bad = 0;
  for (int w = S.work_ptr[list]; w < S.work_ptr[list + 1]; w++) {
    const int k = S.work_cols[w];
    const int base = S.colptr[k], nb = S.colptr[k + 1] - base;
    const int rb = S.row_ptr[k], nrow = S.row_ptr[k + 1] - rb;
    const bool staged = nrow <= kStageBlocks;
    if (staged) {
      for (int e = t; e < 36 * nrow; e += THREADS) Bs[e / 36][e % 36] = S.L[36 * (size_t)S.row_blk[rb + e / 36] + (e % 36)];
      for (int e = t; e < 6 * nrow; e += THREADS) ys[e / 6][e % 6] = S.y[6 * (size_t)S.row_col[rb + e / 6] + (e % 6)];
      __syncthreads();
      // 1. gather, one thread per (block row, slice)
      const int R = 6 * nb;
      int G = THREADS / R;
      G = G < 1 ? 1 : (G > 8 ? 8 : G);
      for (int item = t; item < R * G; item += THREADS) {  // (one pass unless the column has more than THREADS / 6 blocks)
        const int ri = item / G, g = item % G;
        const int d = base + ri / 6, r = ri % 6;
        const int ub = S.upd_ptr[d], len = S.upd_ptr[d + 1] - ub;
        const int per = (len + G - 1) / G;
        int u = ub + g * per;
        const int ue = min(ub + len, u + per);
        double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        constexpr int kBatch = 4;
        for (; u < ue; u += kBatch) {
          int ia[kBatch], bp[kBatch];
#pragma unroll
          for (int q = 0; q < kBatch; q++) {
            const int uu = u + q < ue ? u + q : ue - 1;
            ia[q] = S.upd_a[uu];
            bp[q] = S.upd_bpos[uu];
          }
          double av[kBatch][6];
#pragma unroll
          for (int q = 0; q < kBatch; q++) {
            const double* A = S.L + 36 * (size_t)ia[q] + r;
#pragma unroll
            for (int m = 0; m < 6; m++) av[q][m] = A[6 * m];
          }
#pragma unroll
          for (int q = 0; q < kBatch; q++)
            if (u + q < ue) {
              const double* B = Bs[bp[q]];
#pragma unroll
              for (int m = 0; m < 6; m++)
#pragma unroll
                for (int c = 0; c < 6; c++) acc[c] -= av[q][m] * B[c + 6 * m];
            }
        }
        if (G == 1 && R <= THREADS) {
          // no slices to meet: the row goes to its place at once
#pragma unroll
          for (int c = 0; c < 6; c++) {
            const double v = S.L[36 * (size_t)d + r + 6 * c] + acc[c];
            if (d == base) D[r][c] = v;
            else S.L[36 * (size_t)d + r + 6 * c] = v;
          }
        } else if (R * G <= THREADS) {
#pragma unroll
          for (int c = 0; c < 6; c++) part[item][c] = acc[c];
        } else {
          // more rows than threads (G == 1, several passes): straight to memory as well
#pragma unroll
          for (int c = 0; c < 6; c++) {
            const double v = S.L[36 * (size_t)d + r + 6 * c] + acc[c];
            if (d == base) D[r][c] = v;
            else S.L[36 * (size_t)d + r + 6 * c] = v;
          }
        }
      }
      // right-hand side of the forward substitution: b_k - sum_j L_kj y_j, sixteen slices of the row list
      if (t < 96) {
        const int r = t % 6, g = t / 6;
        const int per = (nrow + 15) / 16;
        double a = 0.0;
        for (int j = g * per; j < min(nrow, (g + 1) * per); j++)
#pragma unroll
          for (int m = 0; m < 6; m++) a -= Bs[j][r + 6 * m] * ys[j][m];
        rpart[g][r] = a;
      }
      __syncthreads();
      if (G > 1 && R * G <= THREADS) {
        for (int e = t; e < 6 * R; e += THREADS) {
          const int ri = e / 6, c = e % 6;
          const int d = base + ri / 6, r = ri % 6;
          double v = S.L[36 * (size_t)d + r + 6 * c];
          for (int g = 0; g < G; g++) v += part[ri * G + g][c];
          if (d == base) D[r][c] = v;
          else S.L[36 * (size_t)d + r + 6 * c] = v;
        }
      }
      if (t < 6) {
        double a = S.y[6 * (size_t)k + t];
        for (int g = 0; g < 16; g++) a += rpart[g][t];
        rhs[t] = a;
      }
    } else {
      // row list too long for the stage: per-entry gather, as in sparse_factor_kernel
      for (int e = t; e < 36 * nb; e += THREADS) {
        const int d = base + e / 36, r = (e % 36) % 6, c = (e % 36) / 6;
        double acc = S.L[36 * (size_t)d + (e % 36)];
        for (int u = S.upd_ptr[d]; u < S.upd_ptr[d + 1]; u++) {
          const double* A = S.L + 36 * (size_t)S.upd_a[u];
          const double* B = S.L + 36 * (size_t)S.upd_b[u];
#pragma unroll
          for (int q = 0; q < 6; q++) acc -= A[r + 6 * q] * B[c + 6 * q];
        }
        if (d == base) D[r][c] = acc;
        else S.L[36 * (size_t)d + (e % 36)] = acc;
      }
      if (t >= 64 && t < 70) {
        const int r = t - 64;
        double acc = S.y[6 * (size_t)k + r];
        for (int u = rb; u < rb + nrow; u++) {
          const double* A = S.L + 36 * (size_t)S.row_blk[u];
          const double* yj = S.y + 6 * (size_t)S.row_col[u];
#pragma unroll
          for (int q = 0; q < 6; q++) acc -= A[r + 6 * q] * yj[q];
        }
        rhs[r] = acc;
      }
    }
    __syncthreads();
    sparse_column_tail<THREADS>(S, k, base, nb, t, D, rhs, dinv, &bad);
  }
  if (t == 0 && bad) atomicOr(S.status, 1);
}

// backward substitution x_k = L_kk^-T (y_k - sum_i L_ik^T x_i) over the columns of a work list in REVERSE elimination order
__global__ void __launch_bounds__(64) sparse_backsolve_kernel(SparseView S, int first_list) {
  __shared__ double part[6][6], v[6];
  const int list = first_list + blockIdx.x;
  const int t = threadIdx.x;
  for (int w = S.work_ptr[list + 1] - 1; w >= S.work_ptr[list]; w--) {
    const int k = S.work_cols[w];
    const int base = S.colptr[k], nb = S.colptr[k + 1] - base;
    if (t < 36) {
      // lane (c, slice): component c of sum_i L_ik^T x_i over the blocks slice, slice + 6, ... (fixed order)
      const int c = t % 6, slice = t / 6;
      double acc = 0.0;
      for (int p = 1 + slice; p < nb; p += 6) {
        const double* A = S.L + 36 * (size_t)(base + p);
        const double* xi = S.x + 6 * (size_t)S.rowidx[base + p];
#pragma unroll
        for (int q = 0; q < 6; q++) acc += A[q + 6 * c] * xi[q];
      }
      part[slice][c] = acc;
    }
    __syncthreads();
    if (t < 6) {
      double s = S.y[6 * (size_t)k + t];
      for (int sl = 0; sl < 6; sl++) s -= part[sl][t];
      v[t] = s;
    }
    __syncthreads();
    if (t == 0) back6(S.L + 36 * (size_t)base, S.dinv + 6 * (size_t)k, v, S.x + 6 * (size_t)k);
    __syncthreads();  // x_k is read by the next columns of this list (one wave per workgroup: the barrier is free)
  }
}

__global__ void __launch_bounds__(256) sparse_unpermute_kernel(const double* __restrict__ x_elim, const int* __restrict__ perm, int P, double* __restrict__ x_slots) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 6 * P) x_slots[6 * (size_t)perm[i / 6] + i % 6] = x_elim[i];
}

// the last launch of gp_sparse_system_step: x in slot order on the device and where the host reads it, and the status word beside it
__global__ void __launch_bounds__(256) sparse_step_end_kernel(const double* __restrict__ x_elim, const int* __restrict__ perm, int P, double* __restrict__ x_slots,
                                                              double* __restrict__ x_slots_host, const int* __restrict__ status, double* __restrict__ status_host) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < 6 * P) {
    const double v = x_elim[i];
    const size_t to = 6 * (size_t)perm[i / 6] + i % 6;
    x_slots[to] = v;
    x_slots_host[to] = v;
  }
  if (i == 0) *status_host = (double)*status;
}

}  // namespace gp
