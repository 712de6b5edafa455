// gp_sparse_small.hip -- the one-launch damped step of a SMALL graph, a unit of its own behind launch_small_step (the multi-launch kernels of gp_sparse.hip compile to
// other code with this kernel beside them in one module)
#include "gp_host.hpp"
#include "gp_sparse_block6.hpp"
#include "gp_sparse_small.hpp"

namespace gp {

// ---- the damped step of a SMALL graph: the assembly + ONE launch for everything behind it (round 6) -----------------------------------------------------
// The multi-launch step (gp_sparse_multi.hpp) costs 0.21 ms on BASELINE configs[2]'s graph (63 free poses, 256 factors) and its launches are NOT the cost: the kernels' own time is
// (profiles/r06_solver_kernel_stats.csv).  A column of the factorisation is a chain -- product indices -> operand blocks -> 6 x 6 Cholesky -> triangular solves -- and
// every link is a round trip to L2 behind a workgroup barrier.  For a graph whose whole factor fits the LDS of one compute unit (<= ~400 blocks of 288 B; the index
// lists beside it) ONE 512-thread workgroup factors and solves with every operand in LDS:
//   phase 0  the index lists and the ASSEMBLED system (L's blocks, b, the diagonal) from global memory into LDS: coalesced, ~3 us.  The assembly itself stays
//            sparse_assemble_kernel<true>, one 64-lane workgroup per block of L across the whole chip, in the launch in front: it is a gather of 8-byte values out of the
//            factors' records, and ONE compute unit's vector-memory path needs 40 us for it (measured: the first form of this kernel assembled in place, with its lists in
//            LDS and sixteen loads in flight per thread: 30 - 45 us against the assembly kernel's 6.5)
//   phase 1  the schedule's levels one after the other, the work lists of a level side by side (SmallForm::Teams).  Up to four lists in a level -- a team of 8 / lists
//            waves per list, which share a column's gather and meet through LDS words (small_forward_teams; in level 0, the independent subtrees, pipelined:
//            small_forward_pipelined); more lists -- level 0: a list per lone wave (small_forward_lone_waves), levels above (separator chains): a TEAM of 512 / lists
//            threads in lock step (small_forward_lock_step).  SmallForm::LockStep: the lock-step form everywhere, as first built; LoneWaves: lone waves in level 0, lock
//            step above.
//   phase 2  the backward substitution, levels and columns in reverse: a list per wave, no barrier inside a list (LockStep: two barriers per round)
//   phase 3  x in slot order to the device array and the host, the status word
// Every scalar is computed by the SAME sequence of operations as in sparse_factor_kernel<256> (lists of level 0) / sparse_factor_staged_kernel<1024> (levels above: the
// slice partials with G and `per` derived from the column's size exactly as there) / sparse_backsolve_kernel, so the step is bit-identical to the multi-launch form
// (tests/test_solver_gpu.py::test_one_launch_step_is_bit_identical); only where the operands live (row-major blocks in LDS) and which thread computes what differ.

// the index lists in LDS (SparseSmallView::off, in this order)
struct SmallLists { const int *colptr, *rowidx, *upd_ptr, *upd_a, *upd_b, *row_ptr, *row_blk, *row_col, *work_ptr, *work_cols, *blkcol, *list_maxnb; };
// the system in LDS (small_lds_layout) and the workgroup's words
struct SmallLds {
  double *Ls, *ys, *xs, *dis, *d0s, *scr;  // L's blocks, ROW-major | y | x | reciprocals of L's diagonal | the assembled diagonal of A (the pivots' scale) | the teams' scratch
  int* bad;
  unsigned *arrive, *done;  // [kSmallTeams] the teams' handshakes: monotonic within a batch of lists
  unsigned long long* tr;   // [64] the stamps stay in LDS until the end: a store to memory in front of a fence would be waited for, and measured
};
__device__ __forceinline__ void small_stamp(const SmallLds& M, const bool on, const int i) { if (on) M.tr[i] = __builtin_amdgcn_s_memtime(); }

// acc - sum over the products u in [u, ue) of (row r of block upd_a[u]) . (row c of block upd_b[u]), subtracted in list order; operands in LDS.  Four products' indices,
// then their 48 operands, are requested together (one entry's products are a chain of dependent LDS round trips otherwise: 800 clocks per product measured)
__device__ __forceinline__ double small_sub_products(double acc, const SmallLists& I, int u, const int ue, const double* Ls, const int r, const int c) {
  constexpr int kBatch = 4;
  for (; u < ue; u += kBatch) {
    int ia[kBatch], ib[kBatch];
#pragma unroll
    for (int w = 0; w < kBatch; w++) {
      const int uu = u + w < ue ? u + w : ue - 1;  // (a short tail repeats the last product's operands and skips its subtraction)
      ia[w] = I.upd_a[uu];
      ib[w] = I.upd_b[uu];
    }
    double av[kBatch][6], bv[kBatch][6];
#pragma unroll
    for (int w = 0; w < kBatch; w++) {
      load_row6(Ls + 36 * (size_t)ia[w] + 6 * r, av[w]);
      load_row6(Ls + 36 * (size_t)ib[w] + 6 * c, bv[w]);
    }
#pragma unroll
    for (int w = 0; w < kBatch; w++)
      if (u + w < ue) {
#pragma unroll
        for (int q = 0; q < 6; q++) acc -= av[w][q] * bv[w][q];
      }
  }
  return acc;
}

// ---- the panel of a column, a ROW per lane, swept right-looking pivot by pivot ---------------------------------------------------------------------------------------
// 1 / sqrt(pivot) and the diagonal block's column p are wave-uniform (v_readlane), every row scales its entry p and updates its entries c > p from its own registers.
// Entry by entry that is the SAME sequence of operations on the same operands as chol6_wave (diagonal block), trsm_row6 (blocks below) and forward6 (right-hand side) --
// fma(-x_rp, L_cp, x_rc) for p ascending, then x_rc * (1 / L_cc) -- so the factor is bit-identical to the lock-step form's and the multi-launch kernels'.
// One copy for small_wave_column and small_panel_sweep, as text: the callers declare `double sc[6], rl[6], pl[6], lcp[6][6]; bool any_bad` (sc: the assembled diagonal
// entries the pivots are held against).  As a function over references the same loop cost small_wave_column 28 more VGPRs (214 against 186).
// a: row i of the panel (rows 0-5: the diagonal block); first: the pass of 64 rows that holds the diagonal block -- it derives the pivots' scalars, later passes reuse them
#define GP_SWEEP_PIVOTS6(a, i, first)                                             \
  _Pragma("unroll") for (int p = 0; p < 6; p++) {                                 \
    if (first) {                                                                  \
      double piv = lane_bcast_f64(a[p], p);                                       \
      if (!pivot_ok(piv, sc[p])) {                                                \
        any_bad = true;                                                           \
        piv = 1.0;                                                                \
      }                                                                           \
      rl[p] = rsqrt_f64(piv);                                                     \
      pl[p] = piv * rl[p];                                                        \
    }                                                                             \
    a[p] = (i == p) ? pl[p] : a[p] * rl[p];                                       \
    if (first) {                                                                  \
      _Pragma("unroll") for (int c = 0; c < 6; c++)                               \
        if (c > p) lcp[c][p] = lane_bcast_f64(a[p], c);                           \
    }                                                                             \
    _Pragma("unroll") for (int c = 0; c < 6; c++)                                 \
      if (c > p) a[c] = __builtin_fma(-a[p], lcp[c][p], a[c]);                    \
  }

// ---- a column by ONE wave (round 6, second form of the one-launch step) ------------------------------------------------------------------------------------------
// The lock-step form below spends a round's 7900 clocks mostly WAITING: three workgroup barriers, one wave factoring the diagonal block while the others idle, lanes
// exchanging entries through LDS.  Here a work list belongs to one wave, which walks its columns with no barrier at all (the next column's operands were written by the
// same wave), and a lane owns a whole ROW of the column's panel -- lanes 0-5 the rows of the diagonal block, lanes 6-11 the six entries of the forward substitution's
// right-hand side while they are gathered (then lane 6 holds them as one row), lanes 12.. the rows of the blocks below -- with its six entries in registers:
//  1. gather: lane (row r of block d) subtracts, product by product in list order, (row r of block upd_a) . (row c of block upd_b) for its six c; the right-hand-side
//     lanes run the same loop over the row list with y in the place of block upd_b (one "row").  Per entry: the lock-step form's and the multi-launch kernels' arithmetic.
//  2. the panel is swept (GP_SWEEP_PIVOTS6).  More than 52 rows below the diagonal: further passes of 64 rows with the pivots' scalars kept.
// Measured (scripts/r06/solver_trace.py, BASELINE configs[2]'s graph: two lists of 29 / 30 columns): a column 6600 clocks (gather 3700, panel 1550, write-back 1050)
// against the lock-step form's 7900; a lone wave issues an instruction every ~4.5 clocks whatever it is, so what a column costs is its instruction count.  Three
// re-formulations of the gather were built and measured no better -- entries dealt three to a lane (4900 clocks: the index chain per turn), a static per-lane program of
// operand offsets in device memory (3600; with the next column's words prefetched 4800: the words' way from L2 is longer than a turn) -- and were removed.
__device__ __forceinline__ void small_wave_column(const int k, const int lane, const SmallLds& M, const SmallLists& I, unsigned long long* stamp) {
  double *const Ls = M.Ls, *const ys = M.ys;
  const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
  const int rb = I.row_ptr[k], nrow = I.row_ptr[k + 1] - rb;
  const int rows = 6 * nb + 6;  // 6 (diagonal block) + 6 (right-hand-side entries; lane 6 becomes the row) + 6 (nb - 1)
  double sc[6], rl[6], pl[6], lcp[6][6];
  bool any_bad = false;
#pragma unroll
  for (int p = 0; p < 6; p++) sc[p] = M.d0s[6 * (size_t)k + p];
  for (int c0 = 0; c0 < rows; c0 += 64) {
    const int i = c0 + lane;
    const bool act = i < rows, is_rhs = i >= 6 && i < 12;
    const int ib = i < 12 ? 0 : (i - 12) / 6 + 1;
    const int r = i < 6 ? i : (i < 12 ? i - 6 : (i - 12) % 6);
    const int d = base + ib;
    // ---- gather ----
    double a[6];
    const int* la = is_rhs ? I.row_blk : I.upd_a;
    const int* lb = is_rhs ? I.row_col : I.upd_b;
    int u = !act ? 0 : (is_rhs ? rb : I.upd_ptr[d]);
    const int ue = !act ? 0 : (is_rhs ? rb + nrow : I.upd_ptr[d + 1]);
    const double* bbase = is_rhs ? ys : Ls;
    const int bblock = is_rhs ? 6 : 36, brow = is_rhs ? 0 : 6;  // doubles between the "blocks" / rows of the second operand (y: one row)
    if (act && !is_rhs) {
      load_row6(Ls + 36 * (size_t)d + 6 * r, a);
    } else {
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] = 0.0;
      if (act) a[0] = ys[6 * (size_t)k + r];
    }
    constexpr int kBatch = 2;
    for (; u < ue; u += kBatch) {
      double av[kBatch][6], bv[kBatch][6][6];
#pragma unroll
      for (int w = 0; w < kBatch; w++) {
        const int uu = u + w < ue ? u + w : ue - 1;  // (a short tail repeats the last product's operands and skips its subtraction)
        load_row6(Ls + 36 * (size_t)la[uu] + 6 * r, av[w]);
        const double* Bb = bbase + (size_t)bblock * lb[uu];
#pragma unroll
        for (int c = 0; c < 6; c++) load_row6(Bb + brow * c, bv[w][c]);
      }
#pragma unroll
      for (int w = 0; w < kBatch; w++)
        if (u + w < ue) {
#pragma unroll
          for (int c = 0; c < 6; c++) {
#pragma unroll
            for (int q = 0; q < 6; q++) a[c] -= av[w][q] * bv[w][c][q];
          }
        }
    }
    if (c0 == 0) {
      // the right-hand side's six entries (lanes 6-11, entry 0 each) become lane 6's row
      double rh[6];
#pragma unroll
      for (int q = 0; q < 6; q++) rh[q] = lane_bcast_f64(a[0], 6 + q);
      if (lane == 6) {
#pragma unroll
        for (int q = 0; q < 6; q++) a[q] = rh[q];
      }
    }
    if (stamp && c0 == 0) stamp[1] = __builtin_amdgcn_s_memtime();
    GP_SWEEP_PIVOTS6(a, i, c0 == 0)
    if (stamp && c0 == 0) stamp[2] = __builtin_amdgcn_s_memtime();
    // ---- back to LDS ----
    if (act && i < 6) {
#pragma unroll
      for (int c = 0; c < 6; c++) Ls[36 * (size_t)base + 6 * r + c] = c <= r ? a[c] : 0.0;
    } else if (act && i == 6) {
#pragma unroll
      for (int c = 0; c < 6; c++) ys[6 * (size_t)k + c] = a[c];
    } else if (act && i >= 12) {
#pragma unroll
      for (int c = 0; c < 6; c++) Ls[36 * (size_t)d + 6 * r + c] = a[c];
    }
    if (c0 == 0 && lane == 7) {
#pragma unroll
      for (int p = 0; p < 6; p++) M.dis[6 * (size_t)k + p] = rl[p];
    }
  }
  if (any_bad && lane == 0) *M.bad = 1;
  GP_WAVE_SYNC_LDS();  // (the next column of this wave reads what its other lanes have just written)
  if (stamp) stamp[3] = __builtin_amdgcn_s_memtime();
}

// ---- a column by a TEAM of waves without workgroup barriers (the product where a level has at most four lists) ---------------------------------------------------------
// What a lone wave's column costs is its instruction count, and 3700 of its 6400 clocks are the gather.  Here the gather is dealt ENTRY by entry over the G >= 2 waves of
// the list's team (G = 8 / lists: BASELINE configs[2]'s two lists get four waves each; one entry per lane, its products subtracted in list order in place -- the lock-step
// form's arithmetic: small_sub_products; the right-hand side's six entries on the team's last wave, beside the blocks' entries, not behind them), the waves meet at a
// counter in LDS, the team's first wave sweeps the panel row by row (small_panel_sweep) and releases the others through a sequence word.
// No s_barrier: the other lists' teams run on at their own pace (all eight waves are resident: a wave that polls never keeps the wave it waits for from running).
// Measured (scripts/r06/solver_forms.py, solver_trace.py): a column 6400 -> 4100 clocks (gather + meeting 1850, sweep 1850, release 160), the kernel 276 k -> 245 k;
// pipelined (the other waves start the next column's older products during the sweep) 3650 clocks, 235 k.

// the forward substitution's right-hand side of column k, entry r, to *dst: b_k[r] - sum over the row list of L_kj[r, :] . y_j, in list order.  Four blocks of the row are
// requested together (one at a time every block is two dependent LDS round trips + six dependent multiply-adds on the column's critical path)
__device__ __forceinline__ void small_rhs_gather(const int k, const int r, const SmallLds& M, const SmallLists& I, double* dst) {
  double acc = M.ys[6 * (size_t)k + r];
  int u = I.row_ptr[k];
  const int ue = I.row_ptr[k + 1];
  for (; u < ue; u += 4) {
    int ib[4], ic[4];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      const int uu = u + w < ue ? u + w : ue - 1;
      ib[w] = I.row_blk[uu];
      ic[w] = I.row_col[uu];
    }
    double av[4][6], yv[4][6];
#pragma unroll
    for (int w = 0; w < 4; w++) {
      load_row6(M.Ls + 36 * (size_t)ib[w] + 6 * r, av[w]);
      load_row6(M.ys + 6 * (size_t)ic[w], yv[w]);
    }
#pragma unroll
    for (int w = 0; w < 4; w++)
      if (u + w < ue) {
#pragma unroll
        for (int q = 0; q < 6; q++) acc -= av[w][q] * yv[w][q];
      }
  }
  *dst = acc;
}
// STAGED: the column belongs to a level above 0 -- the sums are those of sparse_factor_staged_kernel<1024>: an entry's product list in G contiguous slices, each summed
// from zero, met in slice order (G = clamp(1024 / (6 blocks), 1, 8), `per` as there) ...
__device__ __forceinline__ double small_staged_entry(double v, const int d, const int nb, const int r, const int c, const double* Ls, const SmallLists& I) {
  int G = 1024 / (6 * nb);
  G = G < 1 ? 1 : (G > 8 ? 8 : G);
  const int ub = I.upd_ptr[d], ulen = I.upd_ptr[d + 1] - ub;
  const int per = (ulen + G - 1) / G;
  for (int g = 0; g < G; g++) {
    const double acc = small_sub_products(0.0, I, ub + g * per, min(ub + ulen, ub + g * per + per), Ls, r, c);
    v += acc;
  }
  return v;
}
// ... and the right-hand side's row list in sixteen such slices: slice g of entry r, summed from zero
__device__ __forceinline__ double small_staged_rhs_slice(const int k, const int r, const int g, const SmallLds& M, const SmallLists& I) {
  const int rb = I.row_ptr[k], nrow = I.row_ptr[k + 1] - rb;
  const int per = (nrow + 15) / 16;
  double a = 0.0;
  for (int q = g * per; q < min(nrow, (g + 1) * per); q++) {
    const double* A = M.Ls + 36 * (size_t)I.row_blk[rb + q] + 6 * r;
    const double* yj = M.ys + 6 * (size_t)I.row_col[rb + q];
#pragma unroll
    for (int m = 0; m < 6; m++) a -= A[m] * yj[m];
  }
  return a;
}
// the gather of column k by wave wt of a team of G
template <bool STAGED>
__device__ __forceinline__ void small_entry_gather(const int k, const int wt, const int G, const int lane, const SmallLds& M, const SmallLists& I) {
  const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
  // the blocks' entries: one per lane, wave by wave
  for (int e = wt * 64 + lane; e < 36 * nb; e += 64 * G) {
    const int d = base + e / 36, r = (e % 36) % 6, c = (e % 36) / 6;
    double* dst = M.Ls + 36 * (size_t)d + 6 * r + c;
    *dst = STAGED ? small_staged_entry(*dst, d, nb, r, c, M.Ls, I) : small_sub_products(*dst, I, I.upd_ptr[d], I.upd_ptr[d + 1], M.Ls, r, c);
  }
  // the right-hand side's six entries: the team's LAST wave, lanes 58-63 (another instruction stream than the blocks' entries: beside them, where that wave holds none --
  // a column of five blocks leaves the fourth wave of four free --, not behind them)
  if (wt == G - 1 && lane >= 58) {
    const int r = lane - 58;
    double* dst = M.ys + 6 * (size_t)k + r;
    if constexpr (!STAGED) {
      small_rhs_gather(k, r, M, I, dst);
    } else {
      double t = *dst;
      for (int g = 0; g < 16; g++) t += small_staged_rhs_slice(k, r, g, M, I);
      *dst = t;
    }
  }
}
// what the sweep of a column reads that does not depend on the gather: requested by the caller BEFORE it waits for the gathering waves
struct SmallSweepHead { int base, nb; double sc[6]; };  // (sc: the assembled diagonal entries the pivots are held against)
__device__ __forceinline__ SmallSweepHead small_sweep_head(const int k, const SmallLds& M, const SmallLists& I) {
  SmallSweepHead h;
  h.base = I.colptr[k];
  h.nb = I.colptr[k + 1] - h.base;
  load_row6(M.d0s + 6 * (size_t)k, h.sc);
  return h;
}
// the gathered panel of column k, row by row (lanes 0-5 the diagonal block, lane 6 the right-hand side, lanes 7.. the rows of the blocks below): small_wave_column's sweep
__device__ __forceinline__ void small_panel_sweep(const int k, const SmallSweepHead& head, const int lane, const SmallLds& M) {
  const int base = head.base, nb = head.nb;
  const int rows = 6 * nb + 1;
  double sc[6], rl[6], pl[6], lcp[6][6];
  bool any_bad = false;
#pragma unroll
  for (int p = 0; p < 6; p++) sc[p] = head.sc[p];
  for (int c0 = 0; c0 < rows; c0 += 64) {
    const int i = c0 + lane;
    const bool act = i < rows;
    const int ib = i < 7 ? 0 : (i - 7) / 6 + 1;
    const int r = i < 6 ? i : (i < 7 ? 0 : (i - 7) % 6);
    double* row = i == 6 ? M.ys + 6 * (size_t)k : M.Ls + 36 * (size_t)(base + ib) + 6 * r;
    double a[6];
    if (act) {
      load_row6(row, a);
    } else {
#pragma unroll
      for (int c = 0; c < 6; c++) a[c] = 0.0;
    }
    GP_SWEEP_PIVOTS6(a, i, c0 == 0)
#pragma unroll
    for (int c = 1; c < 6; c++) a[c] = (i < c) ? 0.0 : a[c];  // (rows 0-5 of the first pass: the diagonal block's upper triangle is stored as zeros)
    if (act) store_row6(row, a);
    if (c0 == 0 && lane < 6) {
      double v = rl[0];
#pragma unroll
      for (int p = 1; p < 6; p++) v = lane == p ? rl[p] : v;
      M.dis[6 * (size_t)k + lane] = v;
    }
  }
  if (any_bad && lane == 0) *M.bad = 1;
}

// backward substitution of a column by ONE wave: the lock-step form's operations (six slices of the blocks below, met in slice order, then back6) without its barriers
__device__ __forceinline__ void small_wave_back_column(const int k, const int lane, const SmallLds& M, const SmallLists& I, double* scratch /* [48]: this wave's */) {
  const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
  double (*bpart)[6] = reinterpret_cast<double (*)[6]>(scratch);
  if (lane < 36) {
    const int c = lane % 6, slice = lane / 6;
    double acc = 0.0;
    for (int p = 1 + slice; p < nb; p += 6) {
      const double* A = M.Ls + 36 * (size_t)(base + p);
      const double* xi = M.xs + 6 * (size_t)I.rowidx[base + p];
#pragma unroll
      for (int q = 0; q < 6; q++) acc += A[6 * q + c] * xi[q];
    }
    bpart[slice][c] = acc;
  }
  GP_WAVE_SYNC_LDS();
  double sum = 0.0;
  if (lane < 6) {
    sum = M.ys[6 * (size_t)k + lane];
    for (int sl = 0; sl < 6; sl++) sum -= bpart[sl][lane];
  }
  // (the six sums go to lane 0 through v_readlane instead of through LDS: one write, one fence and one read less on every column's chain)
  double v[6];
#pragma unroll
  for (int q = 0; q < 6; q++) v[q] = lane_bcast_f64(sum, q);
  if (lane == 0) back6<true>(M.Ls + 36 * (size_t)base, M.dis + 6 * (size_t)k, v, M.xs + 6 * (size_t)k);
  GP_WAVE_SYNC_LDS();
}

// ---- the forward forms: a batch of nb_lists <= kSmallTeams work lists of one level, from list `first` on; tr0: thread 0 stamps this batch's first rounds -------------------

// Teams, pipelined (level 0; every column of the list leaves the team's first wave free of entries: 36 nb <= 64 (G - 1)): the first wave gathers the right-hand side and
// sweeps; the others gather the blocks' entries -- and, while the first wave sweeps column k, already the products of the NEXT column that do not come from column k
// (only the previous column of the list can still be in the making: every other source column was swept before it); the product from column k, last in its
// list, follows when the sweep is released.  Same products in the same order per entry: the same bits.
__device__ __forceinline__ void small_forward_pipelined(const int list, const int team, const int wt, const int G, const int lane, const bool tr0, const SmallLds& M, const SmallLists& I) {
  const int wb = I.work_ptr[list], we = I.work_ptr[list + 1];
  double* const Ls = M.Ls;
  if (wt == 0) {
    unsigned seq = 0;
    int rd = 0;
    for (int w = wb; w < we; w++, rd++) {
      const int k = I.work_cols[w];
      const bool st = tr0 && rd < 14;
      small_stamp(M, st, 8 + 4 * rd);
      if (lane >= 58) small_rhs_gather(k, lane - 58, M, I, M.ys + 6 * (size_t)k + (lane - 58));
      GP_WAVE_SYNC_LDS();
      seq++;
      const SmallSweepHead head = small_sweep_head(k, M, I);
      while (__hip_atomic_load(&M.arrive[team], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq * (unsigned)(G - 1)) __builtin_amdgcn_s_sleep(1);
      small_stamp(M, st, 8 + 4 * rd + 1);
      small_panel_sweep(k, head, lane, M);
      GP_WAVE_SYNC_LDS();
      small_stamp(M, st, 8 + 4 * rd + 2);
      if (lane == 0) __hip_atomic_store(&M.done[team], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      small_stamp(M, st, 8 + 4 * rd + 3);
    }
  } else {
    const int e = (wt - 1) * 64 + lane;
    double acc = 0.0;
    bool started = false;  // the entry's value and its older products are already in acc
    unsigned seq = 0;
    for (int w = wb; w < we; w++) {
      const int k = I.work_cols[w], kprev = w > wb ? I.work_cols[w - 1] : -1;
      const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
      const bool mine = e < 36 * nb;
      const int d = base + (mine ? e / 36 : 0), r = (e % 36) % 6, c = (e % 36) / 6;
      double* dst = Ls + 36 * (size_t)d + 6 * r + c;
      const int u0 = I.upd_ptr[d], ue = I.upd_ptr[d + 1];
      const bool tail = mine && ue > u0 && I.blkcol[I.upd_a[ue - 1]] == kprev;  // the last product comes from the column in the making
      if (mine && !started) acc = small_sub_products(*dst, I, u0, ue - (tail ? 1 : 0), Ls, r, c);
      if (seq > 0)
        while (__hip_atomic_load(&M.done[team], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq) __builtin_amdgcn_s_sleep(1);
      if (tail) acc = small_sub_products(acc, I, ue - 1, ue, Ls, r, c);
      if (mine) *dst = acc;
      GP_WAVE_SYNC_LDS();
      seq++;
      if (lane == 0) __hip_atomic_fetch_add(&M.arrive[team], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
      started = false;
      if (w + 1 < we) {  // the next column's older products, while the first wave sweeps this one
        const int kn = I.work_cols[w + 1];
        const int bn = I.colptr[kn], nbn = I.colptr[kn + 1] - bn;
        if (e < 36 * nbn) {
          const int dn = bn + e / 36;
          const int v0 = I.upd_ptr[dn], ve = I.upd_ptr[dn + 1];
          const bool tn = ve > v0 && I.blkcol[I.upd_a[ve - 1]] == k;
          acc = small_sub_products(Ls[36 * (size_t)dn + 6 * r + c], I, v0, ve - (tn ? 1 : 0), Ls, r, c);
        }
        started = true;
      }
    }
  }
}
// Teams (any level): gather by all G waves of the list's team (small_entry_gather), panel sweep by the first (small_panel_sweep), two LDS handshakes per column
__device__ __forceinline__ void small_forward_teams(const int list, const bool staged, const int team, const int wt, const int G, const int lane, const bool tr0, const SmallLds& M,
                                                    const SmallLists& I) {
  unsigned seq = 0;
  int rd = 0;
  for (int w = I.work_ptr[list]; w < I.work_ptr[list + 1]; w++, rd++) {
    const int k = I.work_cols[w];
    const bool st = tr0 && rd < 14;
    small_stamp(M, st, 8 + 4 * rd);
    if (staged) small_entry_gather<true>(k, wt, G, lane, M, I);
    else small_entry_gather<false>(k, wt, G, lane, M, I);
    GP_WAVE_SYNC_LDS();
    seq++;
    if (lane == 0) __hip_atomic_fetch_add(&M.arrive[team], 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (wt == 0) {
      const SmallSweepHead head = small_sweep_head(k, M, I);
      while (__hip_atomic_load(&M.arrive[team], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq * (unsigned)G) __builtin_amdgcn_s_sleep(1);
      small_stamp(M, st, 8 + 4 * rd + 1);
      small_panel_sweep(k, head, lane, M);
      GP_WAVE_SYNC_LDS();
      small_stamp(M, st, 8 + 4 * rd + 2);
      if (lane == 0) __hip_atomic_store(&M.done[team], seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
    } else {
      while (__hip_atomic_load(&M.done[team], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP) < seq) __builtin_amdgcn_s_sleep(1);
    }
    small_stamp(M, st, 8 + 4 * rd + 3);
  }
}
// LoneWaves (level 0): a work list per WAVE, no barrier between its columns (small_wave_column)
__device__ __forceinline__ void small_forward_lone_waves(const int first, const int nb_lists, const int t, const bool tr0, const SmallLds& M, const SmallLists& I) {
  const int wv = t >> 6;
  if (wv >= nb_lists) return;
  const int list = first + wv;
  int rd = 0;
  for (int w = I.work_ptr[list]; w < I.work_ptr[list + 1]; w++, rd++) {
    unsigned long long* st = tr0 && rd < 14 ? M.tr + 8 + 4 * rd : nullptr;
    if (st) st[0] = __builtin_amdgcn_s_memtime();
    small_wave_column(I.work_cols[w], t & 63, M, I, st);
  }
}

// LockStep: a TEAM of 512 / lists threads (whole waves) per list, round rd = the rd-th column of every list (backward: from the list's end); thread j of the team
struct SmallTeam {
  int T, j, w0, len, rounds;  // threads per team | this thread in its team | the list's columns: work_cols[w0 .. w0 + len) | the longest list of the batch
  bool member;                // (512 / lists is not always a whole number of waves: the threads left over belong to no list)
  double* S;                  // the team's scratch [kSmallTeamDoubles]: D[6][7] at 0, rhs at 42, v at 48, rpart / bpart at 56, dinv at 152
};
__device__ __forceinline__ SmallTeam small_team(const int t, const int first, const int nb_lists, const SmallLds& M, const SmallLists& I) {
  SmallTeam m;
  m.T = (kSmallThreads / nb_lists) & ~63;
  const int team = t / m.T;
  m.j = t % m.T;
  m.member = team < nb_lists;
  const int list = first + (m.member ? team : 0);
  m.w0 = I.work_ptr[list];
  m.len = m.member ? I.work_ptr[list + 1] - m.w0 : 0;
  m.rounds = 0;
  for (int q = 0; q < nb_lists; q++) m.rounds = max(m.rounds, I.work_ptr[first + q + 1] - I.work_ptr[first + q]);
  m.S = M.scr + (size_t)(m.member ? team : 0) * kSmallTeamDoubles;
  return m;
}
// a round: gather, barrier, 6 x 6 Cholesky + forward substitution by the team's first wave, barrier, the blocks below, barrier
__device__ __forceinline__ void small_forward_lock_step(const int first, const int nb_lists, const bool staged, const int t, const bool tr0, const SmallLds& M, const SmallLists& I) {
  const SmallTeam m = small_team(t, first, nb_lists, M, I);
  const int T = m.T, j = m.j;
  double* const Ls = M.Ls;
  double (*D)[7] = reinterpret_cast<double (*)[7]>(m.S);
  double* rhs = m.S + 42;
  double (*rpart)[6] = reinterpret_cast<double (*)[6]>(m.S + 56);
  double* dinv = m.S + 152;
  for (int rd = 0; rd < m.rounds; rd++) {
    const bool on = m.member && rd < m.len;
    const int k = on ? I.work_cols[m.w0 + rd] : 0;
    const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
    const bool st = tr0 && rd < 14;
    small_stamp(M, st, 8 + 4 * rd);
    if (on) {
      // 1. gather: one thread per entry of the column's blocks; the right-hand side of the forward substitution
      // (measured and removed, round 6: letting the team's idle waves subtract the next column's products of all source columns but this one while the first wave
      //  factors the diagonal block -- bit-identical, and no faster: a round's gather is ~2300 clocks with NO products at all)
      // (one loop per kind of sum: with `staged` tested inside one loop this form measured 1 - 3 % slower)
      if (!staged) {
        for (int e = j; e < 36 * nb; e += T) {
          const int d = base + e / 36, r = (e % 36) % 6, c = (e % 36) / 6;
          double* dst = Ls + 36 * (size_t)d + 6 * r + c;
          const double v = small_sub_products(*dst, I, I.upd_ptr[d], I.upd_ptr[d + 1], Ls, r, c);
          if (d == base) D[r][c] = v;
          else *dst = v;
        }
        if (j < 6) small_rhs_gather(k, j, M, I, rhs + j);
      } else {
        for (int e = j; e < 36 * nb; e += T) {
          const int d = base + e / 36, r = (e % 36) % 6, c = (e % 36) / 6;
          double* dst = Ls + 36 * (size_t)d + 6 * r + c;
          const double v = small_staged_entry(*dst, d, nb, r, c, Ls, I);
          if (d == base) D[r][c] = v;
          else *dst = v;
        }
        for (int jj = j; jj < 96; jj += T) rpart[jj / 6][jj % 6] = small_staged_rhs_slice(k, jj % 6, jj / 6, M, I);  // (a team may be one wave: 64 threads)
      }
    }
    __syncthreads();
    small_stamp(M, st, 8 + 4 * rd + 1);
    // 2. the diagonal block: 6 x 6 Cholesky by the team's first wave (lane = (row, column)), then y_k = L_kk^-1 rhs
    if (on && j < 64) {
      if (staged && j < 6) {
        double a = M.ys[6 * (size_t)k + j];
        for (int g = 0; g < 16; g++) a += rpart[g][j];
        rhs[j] = a;
      }
      GP_WAVE_SYNC_LDS();  // (rhs is complete before lane 0 reads it)
      chol6_wave(D, dinv, j, M.bad, M.d0s + 6 * (size_t)k);
      if (j == 0) forward6(D, dinv, rhs);
    }
    __syncthreads();
    small_stamp(M, st, 8 + 4 * rd + 2);
    if (on) {
      if (j < 36) Ls[36 * (size_t)base + 6 * (j % 6) + j / 6] = (j % 6) >= (j / 6) ? D[j % 6][j / 6] : 0.0;
      if (j >= 36 && j < 42) M.ys[6 * (size_t)k + (j - 36)] = rhs[j - 36];
      if (j >= 42 && j < 48) M.dis[6 * (size_t)k + (j - 42)] = dinv[j - 42];
      // 3. the blocks below: L_ik = B_ik L_kk^-T, one thread per (block, row)
      for (int e = j; e < 6 * (nb - 1); e += T) trsm_row6<true>(Ls + 36 * (size_t)(base + 1 + e / 6), e % 6, D, dinv);
    }
    __syncthreads();
    small_stamp(M, st, 8 + 4 * rd + 3);
  }
}
// a round of the backward substitution: six slices of the blocks below, barrier, met in slice order + back6 by one lane, barrier
__device__ __forceinline__ void small_backward_lock_step(const int first, const int nb_lists, const int t, const SmallLds& M, const SmallLists& I) {
  const SmallTeam m = small_team(t, first, nb_lists, M, I);
  const int j = m.j;
  double* vv = m.S + 48;
  double (*bpart)[6] = reinterpret_cast<double (*)[6]>(m.S + 56);
  for (int rd = 0; rd < m.rounds; rd++) {
    const bool on = m.member && rd < m.len;
    const int k = on ? I.work_cols[m.w0 + m.len - 1 - rd] : 0;
    const int base = I.colptr[k], nb = I.colptr[k + 1] - base;
    if (on && j < 36) {
      const int c = j % 6, slice = j / 6;
      double acc = 0.0;
      for (int p = 1 + slice; p < nb; p += 6) {
        const double* A = M.Ls + 36 * (size_t)(base + p);
        const double* xi = M.xs + 6 * (size_t)I.rowidx[base + p];
#pragma unroll
        for (int q = 0; q < 6; q++) acc += A[6 * q + c] * xi[q];
      }
      bpart[slice][c] = acc;
    }
    __syncthreads();
    if (on && j < 64) {
      if (j < 6) {
        double sum = M.ys[6 * (size_t)k + j];
        for (int sl = 0; sl < 6; sl++) sum -= bpart[sl][j];
        vv[j] = sum;
      }
      GP_WAVE_SYNC_LDS();
      if (j == 0) back6<true>(M.Ls + 36 * (size_t)base, M.dis + 6 * (size_t)k, vv, M.xs + 6 * (size_t)k);
    }
    __syncthreads();
  }
}

__global__ void __launch_bounds__(kSmallThreads) sparse_small_step_kernel(const SparseSmallView V, int* __restrict__ status) {
  extern __shared__ __attribute__((aligned(16))) double small_lds[];
  __shared__ int bad;
  __shared__ unsigned team_arrive[kSmallTeams], team_done[kSmallTeams];
  __shared__ unsigned long long tr_lds[64];
  const SmallLdsLayout lay = small_lds_layout((size_t)V.P, (size_t)V.nnzL, 0);
  const SmallLds M = {small_lds, small_lds + lay.ys, small_lds + lay.xs, small_lds + lay.dis, small_lds + lay.d0s, small_lds + lay.scr, &bad, team_arrive, team_done, tr_lds};
  int* idx = reinterpret_cast<int*>(small_lds + lay.idx);
  const SmallLists I = {idx + V.off[0], idx + V.off[1], idx + V.off[2], idx + V.off[3], idx + V.off[4],  idx + V.off[5],
                        idx + V.off[6], idx + V.off[7], idx + V.off[8], idx + V.off[9], idx + V.off[10], idx + V.off[11]};
  const int t = threadIdx.x;
  const bool tracer = V.trace && t == 0;
  // ---- phase 0 ----
  if (V.trace && t < 64) tr_lds[t] = 0;
  __syncthreads();
  small_stamp(M, tracer, 0);
  if (t == 0) bad = 0;
  for (int i = t; i < V.arena_words; i += kSmallThreads) idx[i] = V.arena[i];
  // the assembled system, written by sparse_assemble_kernel<true> in the launch in front of this one (b and c are already with the host): L's blocks -- column-major in
  // global memory, ROW-major in this copy --, b, and the assembled diagonal the pivots are held against.  Coalesced 8-byte reads, four in flight per thread.
  {
    const int nL = 36 * V.nnzL;
#pragma unroll 4
    for (int i = t; i < nL; i += kSmallThreads) {
      const int blk = i / 36, e = i % 36;
      M.Ls[36 * (size_t)blk + 6 * (e % 6) + e / 6] = V.L_global[i];
    }
    for (int i = t; i < 6 * V.P; i += kSmallThreads) {
      M.ys[i] = V.y_global[i];
      M.d0s[i] = V.diag0_global[i];
    }
  }
  __syncthreads();
  small_stamp(M, tracer, 5);  // lists and system are in LDS
  small_stamp(M, tracer, 1);
  // ---- phase 1: factorisation + forward substitution ----
  for (int lvl = 0; lvl < V.num_levels; lvl++) {
    const int lvl_first = V.level_ptr[lvl], nlists = V.level_ptr[lvl + 1] - lvl_first;
    const bool staged = lvl > 0;
    for (int b0 = 0; b0 < nlists; b0 += kSmallTeams) {  // (more than eight lists in a level: eight at a time)
      const int first = lvl_first + b0, nb_lists = min(kSmallTeams, nlists - b0);
      const bool tr0 = tracer && lvl == 0 && b0 == 0;
      if (V.form == SmallForm::Teams && nb_lists <= kSmallThreads / 128) {
        // up to four lists side by side: a team of G >= 2 waves per list, no workgroup barrier inside the batch (teams that take different paths meet at its end)
        const int G = (kSmallThreads / 64) / nb_lists;
        const int wv = t >> 6, team = wv / G, wt = wv % G, lane = t & 63;
        if (t < kSmallTeams) team_arrive[t] = 0, team_done[t] = 0;
        __syncthreads();
        const bool pipe = !staged && G >= 2 && team < nb_lists && 36 * I.list_maxnb[first + (team < nb_lists ? team : 0)] <= 64 * (G - 1);
        if (pipe) small_forward_pipelined(first + team, team, wt, G, lane, tr0, M, I);
        else if (team < nb_lists) small_forward_teams(first + team, staged, team, wt, G, lane, tr0, M, I);
      } else if (!staged && V.form != SmallForm::LockStep) {
        small_forward_lone_waves(first, nb_lists, t, tr0, M, I);
      } else {
        small_forward_lock_step(first, nb_lists, staged, t, tr0, M, I);
        continue;  // (its last round ended at a barrier)
      }
      __syncthreads();
    }
  }
  small_stamp(M, tracer, 2);
  // ---- phase 2: backward substitution, levels and columns in reverse ----
  for (int lvl = V.num_levels - 1; lvl >= 0; lvl--) {
    const int lvl_first = V.level_ptr[lvl], nlists = V.level_ptr[lvl + 1] - lvl_first;
    for (int b0 = 0; b0 < nlists; b0 += kSmallTeams) {
      const int first = lvl_first + b0, nb_lists = min(kSmallTeams, nlists - b0);
      if (V.form == SmallForm::LockStep) {
        small_backward_lock_step(first, nb_lists, t, M, I);
        continue;
      }
      const int wv = t >> 6;
      if (wv < nb_lists)
        for (int w = I.work_ptr[first + wv + 1] - 1; w >= I.work_ptr[first + wv]; w--)
          small_wave_back_column(I.work_cols[w], t & 63, M, I, M.scr + (size_t)wv * kSmallTeamDoubles + 56);
      __syncthreads();
    }
  }
  small_stamp(M, tracer, 3);
  // ---- phase 3 ----
  for (int i = t; i < 6 * V.P; i += kSmallThreads) {
    const double v = M.xs[i];
    const size_t to = 6 * (size_t)V.perm[i / 6] + i % 6;
    V.x_slots[to] = v;
    V.x_slots_host[to] = v;
    if (V.has_epi) M.ys[to] = v;  // (y is done with: the epilogue reads x in slot order from here)
  }
  if (V.has_epi) {
    // the trial's poses (gp_lm.hip: lm_poses_kernel's work) while this workgroup still has x at hand: one launch less behind the step
    __syncthreads();
    const int n = V.epi.threads();
    for (int i = t; i < n; i += kSmallThreads) lm_poses_thread(V.epi, i, M.ys, bad != 0);
  }
  if (t == 0) {
    *status = bad;
    *V.status_host = (double)bad;
  }
  small_stamp(M, tracer, 4);
  if (tracer)
    for (int i = 0; i < 64; i++) V.trace[i] = tr_lds[i];
}

// More than 64 KB of dynamic LDS per workgroup has to be asked for; a runtime that refuses leaves the multi-launch step in charge.  The attribute belongs to the
// FUNCTION, not to a system: every system asks for the same ceiling, so that one created later never lowers what an earlier one needs.
bool small_step_available() {
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&sparse_small_step_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)kSmallLdsCeiling) == hipSuccess) return true;
  (void)hipGetLastError();
  return false;
}
void launch_small_step(const SparseSmallView& V, size_t lds_bytes, hipStream_t stream, int* status) {
  hipLaunchKernelGGL(sparse_small_step_kernel, dim3(1), dim3(kSmallThreads), lds_bytes, stream, V, status);
}

}  // namespace gp
