// gp_sparse.hip -- the step after the path, block-sparse: the damped normal equations of a pose
// graph assembled as a block-sparse lower triangle (6x6 blocks = one pose) and solved by a sparse LL^T on the device.
//
// Replaces (reference, host side, on top of GTSAM / Eigen):
//   include/gtsam_points/optimizers/linear_system_builder.hpp:41-72   SparseLinearSystemBuilder<BLOCK_SIZE>: lower-triangular
//                                                                    block-sparse A in a given ordering, b, c
//   src/gtsam_points/optimizers/levenberg_marquardt_ext.cpp:146-161    buildDampedSystem
//   include/gtsam_points/optimizers/linear_solver.hpp:18-30            SparseLinearSolver::solve(A, b)   (called at levenberg_marquardt_ext.cpp:200-220)
//
// This file: gp_sparse_system and its entry points.  The symbolic phase is gp_sparse_symbolic.hip, the multi-launch kernels gp_sparse_multi.hpp, the one-launch step of
// small graphs gp_sparse_small.hip, the 6 x 6 pieces they share gp_sparse_block6.hpp.
//
// Host, once per graph (gp_sparse_symbolic.hip, called by gp_sparse_system_create): elimination order (the slot order of the factor key list, or nested dissection
// by BFS bisection of the pose graph), symbolic factorisation (elimination tree, block structure of L incl. fill), and for every
// block of L the ordered list of block products that update it -- the numeric phase is then a pure GATHER: every block is
// computed by one group of lanes in a fixed order, no atomics, bit-reproducible.
//
// Device, per solve: left-looking block Cholesky scheduled over the elimination tree.  The tree is cut into independent subtrees
// (one workgroup each, columns in elimination order: a column only gathers from its descendants, which are in the same subtree)
// and a top part of separator columns (one workgroup, after the subtrees).  A pose-graph chain ordered by nested dissection
// is ~log2(P) separator columns on top of P / 8-column subtrees; in the natural order it is one path, i.e. one workgroup walking P
// columns.  The forward substitution rides along (y_k is computed when column k is finished); the backward substitution runs
// the same schedule in reverse.  Four launches per solve, whatever the graph (gp_sparse_multi.hpp); a graph whose factor fits one compute
// unit's LDS takes the assembly and ONE launch (gp_sparse_small.hip).
#include <algorithm>
#include <cstring>
#include <numeric>
#include <vector>

#include "gp_damped_step.hpp"
#include "gp_host.hpp"
#include "gp_lm_poses.hpp"
#include "gp_sparse_multi.hpp"
#include "gp_sparse_small.hpp"
#include "gp_sparse_symbolic.hpp"

namespace gp {
// index arrays one behind the other, `pad` zeros behind each; offs[i] = where array i starts
static std::vector<int> pack_int_arrays(std::initializer_list<const std::vector<int>*> arrays, int pad, int* offs) {
  std::vector<int> packed;
  size_t total = 0;
  for (const auto* a : arrays) total += a->size() + (size_t)pad;
  packed.reserve(total + 1);
  for (const auto* a : arrays) {
    *offs++ = (int)packed.size();
    packed.insert(packed.end(), a->begin(), a->end());
    packed.insert(packed.end(), (size_t)pad, 0);
  }
  return packed;
}
}  // namespace gp

struct gp_sparse_system : gp::DampedSystem {
  gp_sparse_system() : gp::DampedSystem("gp_sparse_system") {}
  gp::SparseSymbolic sym;
  std::vector<gp::SparseDest> dests;
  std::vector<gp::Contribution> contribs;
  gp::DeviceArray d_dests, d_contribs, d_int, L, y, x, x_slots, c, status, prior, dinv, diag0;
  gp::SparseView view{};
  const int* d_perm = nullptr;
  // the one-launch step of small graphs (sparse_small_step_kernel): eligible when factor + index lists fit one compute unit's LDS
  bool small_ok = false, one_launch = false;
  std::vector<double> prior_staged;  // the permuted prior diagonal of the step in flight (source of its H2D copy)
  size_t small_lds_bytes = 0;
  gp::DeviceArray d_small_arena, d_level_ptr;
  gp::SparseSmallView small{};
  int issue_step(const gp_linearized6* records_dev, const gp::Damping& damping, const double* prior_diag_host, const gp::LmPoseView* epi, bool* fused) override;
  // the one-launch step (sparse_small_step_kernel): 1 = gp_sparse_system_step uses it when the system qualifies (default), 0 = the multi-launch form; returns what the
  // next step will run.  The two are bit-identical; the switch exists for the test that says so and for A/B timing.  So do 2 and 3, which select the one-launch step's
  // other forms (gp::SmallForm): 2 = LockStep, 3 = LoneWaves.
  int set_one_launch(int enable) override {
    one_launch = enable != 0 && small_ok;
    small.form = enable == 2 ? gp::SmallForm::LockStep : enable == 3 ? gp::SmallForm::LoneWaves : gp::SmallForm::Teams;
    if (!one_launch) return 0;
    return enable == 2 || enable == 3 ? enable : 1;
  }
  // x in slot order and the status word (!= 0: indeterminate, x is not to be used) -- for a consumer queued behind the step on the same stream (the device-side
  // retract of gp_lm.hip)
  void device_solution(const double** x_slots_dev, const int** status_dev) override {
    if (x_slots_dev) *x_slots_dev = x_slots.as<double>();
    if (status_dev) *status_dev = status.as<int>();
  }
};
gp::DampedSystem* gp::as_damped_system(gp_sparse_system_t* s) { return s; }

extern "C" {

int gp_sparse_system_create(int num_slots, const int* factor_slots, int num_factors, int ordering, gp_stream_t stream, gp_sparse_system_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_create: null out");
  *out = nullptr;
  if (num_slots <= 0 || num_factors < 0 || (num_factors > 0 && !factor_slots) || ordering < 0 || ordering > 4)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_create: factor_slots = [num_factors][2] (target, source; < 0 = fixed), ordering 0 .. 4");
  auto s = std::make_unique<gp_sparse_system>();
  GP_TRY(gp::sparse_symbolic(num_slots, factor_slots, num_factors, ordering, &s->sym));
  const gp::SparseSymbolic& S = s->sym;
  const int P = num_slots, nnzL = S.colptr[P];
  s->num_factors = num_factors;
  s->n = 6 * P;
  s->stream = (hipStream_t)stream;
  // block of L -> ordered contribution list, in elimination order; every block of L is a destination: diagonal blocks carry b, fill blocks get an empty list and are
  // written as zeros (no memset per build)
  auto block_of = [&](int i, int k) {
    if (i == k) return S.colptr[k];
    const int* b = S.rowidx.data() + S.colptr[k] + 1;
    const int* e = S.rowidx.data() + S.colptr[k + 1];
    return (int)(std::lower_bound(b, e, i) - S.rowidx.data());
  };
  std::vector<int> all_blocks((size_t)nnzL), diag_of((size_t)nnzL, -1);
  std::iota(all_blocks.begin(), all_blocks.end(), 0);
  for (int k = 0; k < P; k++) diag_of[S.colptr[k]] = k;
  gp::contribution_lists(
      factor_slots, num_factors, S.iperm, all_blocks, block_of, [&](int block, int begin, int count) { return gp::SparseDest{block, diag_of[block], begin, count}; },
      &s->dests, &s->contribs);
  // one device arena for all index arrays (`views` below follows the order they are packed in)
  int offs[12];
  const std::vector<int> packed = gp::pack_int_arrays({&S.colptr, &S.rowidx, &S.upd_ptr, &S.upd_a, &S.upd_b, &S.row_ptr, &S.row_blk, &S.row_col, &S.work_ptr, &S.work_cols, &S.perm, &S.upd_bpos}, 1, offs);
  int rc = GP_OK;
  if ((rc = s->d_int.alloc(sizeof(int) * packed.size())) || (rc = s->d_dests.alloc(sizeof(gp::SparseDest) * s->dests.size())) ||
      (rc = s->d_contribs.alloc(sizeof(gp::Contribution) * std::max<size_t>(s->contribs.size(), 1))) || (rc = s->L.alloc(sizeof(double) * 36 * (size_t)nnzL)) ||
      (rc = s->y.alloc(sizeof(double) * (size_t)s->n)) || (rc = s->x.alloc(sizeof(double) * (size_t)s->n)) || (rc = s->x_slots.alloc(sizeof(double) * (size_t)s->n)) ||
      (rc = s->c.alloc(sizeof(double))) || (rc = s->status.alloc(sizeof(int))) || (rc = s->prior.alloc(sizeof(double) * (size_t)s->n)) ||
      (rc = s->dinv.alloc(sizeof(double) * (size_t)s->n)) || (rc = s->diag0.alloc(sizeof(double) * (size_t)s->n)))
    return rc;
  GP_HIP(hipMemcpy(s->d_int.ptr, packed.data(), sizeof(int) * packed.size(), hipMemcpyHostToDevice));
  GP_HIP(hipMemcpy(s->d_dests.ptr, s->dests.data(), sizeof(gp::SparseDest) * s->dests.size(), hipMemcpyHostToDevice));
  if (!s->contribs.empty()) GP_HIP(hipMemcpy(s->d_contribs.ptr, s->contribs.data(), sizeof(gp::Contribution) * s->contribs.size(), hipMemcpyHostToDevice));
  const int* base = s->d_int.as<int>();
  const int** views[12] = {&s->view.colptr, &s->view.rowidx,  &s->view.upd_ptr,  &s->view.upd_a,     &s->view.upd_b, &s->view.row_ptr,
                           &s->view.row_blk, &s->view.row_col, &s->view.work_ptr, &s->view.work_cols, &s->d_perm,     &s->view.upd_bpos};
  for (int i = 0; i < 12; i++) *views[i] = base + offs[i];
  s->view.L = s->L.as<double>();
  s->view.y = s->y.as<double>();
  s->view.x = s->x.as<double>();
  s->view.dinv = s->dinv.as<double>();
  s->view.diag0 = s->diag0.as<double>();
  s->view.status = s->status.as<int>();
  // the one-launch step (small graphs): its own copy of the index lists it walks, in the order of SmallLists' members, and the levels
  size_t small_words = 0;
  s->small_lds_bytes = gp::small_step_lds_bytes(S, &small_words);
  if (s->small_lds_bytes) {
    std::vector<int> blkcol((size_t)nnzL);
    for (int k = 0; k < P; k++)
      for (int q = S.colptr[k]; q < S.colptr[k + 1]; q++) blkcol[(size_t)q] = k;
    std::vector<int> list_maxnb(S.work_ptr.size() - 1, 0);
    for (size_t l = 0; l + 1 < S.work_ptr.size(); l++)
      for (int w = S.work_ptr[l]; w < S.work_ptr[l + 1]; w++) list_maxnb[l] = std::max(list_maxnb[l], S.colptr[S.work_cols[w] + 1] - S.colptr[S.work_cols[w]]);
    gp::SparseSmallView& V = s->small;
    std::vector<int> arena = gp::pack_int_arrays({&S.colptr, &S.rowidx, &S.upd_ptr, &S.upd_a, &S.upd_b, &S.row_ptr, &S.row_blk, &S.row_col, &S.work_ptr, &S.work_cols, &blkcol, &list_maxnb}, 0, V.off);
    if (arena.size() & 1) arena.push_back(0);
    if (arena.size() > small_words) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_create: internal: the one-launch step's index arena outgrew its estimate");
    if ((rc = s->d_small_arena.alloc(sizeof(int) * std::max<size_t>(arena.size(), 1))) || (rc = s->d_level_ptr.alloc(sizeof(int) * S.level_ptr.size()))) return rc;
    GP_HIP(hipMemcpy(s->d_small_arena.ptr, arena.data(), sizeof(int) * arena.size(), hipMemcpyHostToDevice));
    GP_HIP(hipMemcpy(s->d_level_ptr.ptr, S.level_ptr.data(), sizeof(int) * S.level_ptr.size(), hipMemcpyHostToDevice));
    V.L_global = s->L.as<double>();
    V.y_global = s->y.as<double>();
    V.diag0_global = s->diag0.as<double>();
    V.arena = s->d_small_arena.as<int>();
    V.level_ptr = s->d_level_ptr.as<int>();
    V.arena_words = (int)arena.size(), V.num_levels = (int)S.level_ptr.size() - 1, V.P = P, V.nnzL = nnzL;
    V.perm = s->d_perm;
    V.form = gp::SmallForm::Teams;
    V.x_slots = s->x_slots.as<double>();
    s->small_ok = s->one_launch = gp::small_step_available();
  }
  *out = s.release();
  return GP_OK;
}

// measurement hook: the one-launch step's thread 0 leaves shader-clock stamps in dev_buffer (64 uint64; SparseSmallView::trace); null = off
int gp_debug_sparse_step_trace(gp_sparse_system_t* s, unsigned long long* dev_buffer) {
  if (!s) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_sparse_step_trace: null");
  s->small.trace = dev_buffer;
  return GP_OK;
}

int gp_sparse_system_destroy(gp_sparse_system_t* s) {
  if (!s) return GP_OK;
  (void)hipStreamSynchronize(s->stream);
  delete s;
  return GP_OK;
}

int gp_sparse_system_size(const gp_sparse_system_t* s) { return s ? s->n : 0; }

int gp_sparse_system_info(const gp_sparse_system_t* s, int64_t* nnz_a_blocks, int64_t* nnz_l_blocks, int64_t* block_products, int* num_subtrees, int* top_columns) {
  if (!s) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_info: null");
  const gp::SparseSymbolic& S = s->sym;
  if (nnz_a_blocks) *nnz_a_blocks = S.nnzA;
  if (nnz_l_blocks) *nnz_l_blocks = S.colptr[S.P];
  if (block_products) *block_products = (int64_t)S.upd_a.size();
  if (num_subtrees) *num_subtrees = S.num_subtrees;
  if (top_columns) *top_columns = S.P - S.work_ptr[S.num_subtrees];
  return GP_OK;
}

// a prior diagonal given in slot order, permuted into elimination order (into `staged`, which must outlive the copy) and queued for upload to s->prior
static int upload_prior(gp_sparse_system_t* s, const double* prior_diag_host, std::vector<double>* staged) {
  const gp::SparseSymbolic& S = s->sym;
  staged->resize((size_t)s->n);
  for (int k = 0; k < S.P; k++)
    for (int r = 0; r < 6; r++) (*staged)[6 * (size_t)k + r] = prior_diag_host[6 * (size_t)S.perm[k] + r];
  GP_HIP(hipMemcpyAsync(s->prior.ptr, staged->data(), sizeof(double) * (size_t)s->n, hipMemcpyHostToDevice, s->stream));
  return GP_OK;
}

int gp_sparse_system_build(gp_sparse_system_t* s, const gp_linearized6* records_dev, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal,
                           const double* prior_diag_host) {
  if (!s || (!records_dev && s->num_factors > 0) || !(lambda >= 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_build: bad arguments");
  // (no memsets: the destination list covers every block of L and every entry of y)
  hipLaunchKernelGGL(gp::sparse_assemble_kernel<false>, dim3((unsigned)s->dests.size()), dim3(64), 0, s->stream, s->d_dests.as<gp::SparseDest>(),
                     s->d_contribs.as<gp::Contribution>(), reinterpret_cast<const double*>(records_dev), s->L.as<double>(), s->y.as<double>(), [&] {
                       gp::SparseStepExtras e0{};
                       e0.diag0 = s->diag0.as<double>();
                       return e0;
                     }());
  hipLaunchKernelGGL(gp::sum_errors_kernel<>, dim3(1), dim3(256), 0, s->stream, reinterpret_cast<const double*>(records_dev), s->num_factors, s->c.as<double>());
  const double* prior = nullptr;
  std::vector<double> permuted;
  if (prior_diag_host) {
    GP_TRY(upload_prior(s, prior_diag_host, &permuted));
    prior = s->prior.as<double>();
  }
  if (lambda > 0.0 || prior) {
    hipLaunchKernelGGL(gp::sparse_damp_kernel, dim3((s->n + 255) / 256), dim3(256), 0, s->stream, s->L.as<double>(), s->view.colptr, s->n, lambda, diagonal_damping,
                       min_diagonal, max_diagonal, prior, s->diag0.as<double>());
  }
  GP_HIP(hipGetLastError());
  if (prior_diag_host) GP_HIP(hipStreamSynchronize(s->stream));  // `permuted` goes away
  s->built = true;
  return GP_OK;
}

// the system as a dense symmetric column-major [n][n] in SLOT order (for checkers), b [n] (slot order), c
int gp_sparse_system_download(const gp_sparse_system_t* s, double* A_host, double* b_host, double* c_host) {
  if (!s || !s->built) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_download: build the system first");
  const gp::SparseSymbolic& S = s->sym;
  const size_t n = (size_t)s->n;
  GP_HIP(hipStreamSynchronize(s->stream));
  if (A_host) {
    std::vector<double> L(36 * (size_t)S.colptr[S.P]);
    GP_HIP(hipMemcpy(L.data(), s->L.ptr, sizeof(double) * L.size(), hipMemcpyDeviceToHost));
    std::fill(A_host, A_host + n * n, 0.0);
    for (int k = 0; k < S.P; k++)
      for (int p = S.colptr[k]; p < S.colptr[k + 1]; p++) {
        const int si = S.perm[S.rowidx[p]], sk = S.perm[k];
        for (int c = 0; c < 6; c++)
          for (int r = 0; r < 6; r++) {
            const double v = L[36 * (size_t)p + 6 * c + r];  // A(6 i + r, 6 k + c)
            if (p == S.colptr[k] && r < c) continue;          // diagonal block: lower triangle holds the data
            A_host[(6 * (size_t)sk + c) * n + 6 * (size_t)si + r] = v;
            A_host[(6 * (size_t)si + r) * n + 6 * (size_t)sk + c] = v;
          }
      }
  }
  if (b_host) {
    std::vector<double> y(n);
    GP_HIP(hipMemcpy(y.data(), s->y.ptr, sizeof(double) * n, hipMemcpyDeviceToHost));
    for (int k = 0; k < S.P; k++)
      for (int r = 0; r < 6; r++) b_host[6 * (size_t)S.perm[k] + r] = y[6 * (size_t)k + r];
  }
  if (c_host) GP_HIP(hipMemcpy(c_host, s->c.ptr, sizeof(double), hipMemcpyDeviceToHost));
  return GP_OK;
}

// the numeric phase on the system's stream: factorisation + forward substitution level by level, backward substitution the same levels in reverse
static void launch_factor_and_substitutions(gp_sparse_system_t* s) {
  const gp::SparseSymbolic& S = s->sym;
  // one launch per level of the schedule (level 0: the subtrees; then the chains of separator columns, level by level), the backward
  // substitution the same levels in reverse
  const int levels = (int)S.level_ptr.size() - 1;
  for (int l = 0; l < levels; l++) {
    const int first = S.level_ptr[l], count = S.level_ptr[l + 1] - first;
    // 256 threads for the subtrees (columns of a few blocks), 1024 for the chains of separator columns (a dozen blocks each).  Measured on the 512-pose
    // band graph (profiles/r03_solver_time.txt): this form 1.34 ms; 512 threads + batches of eight products 1.45-1.48 ms with or without the next
    // batch's indices prefetched; 1024 threads + batches of eight 2.8 ms (the 128-register cap spills the batch)
    if (count > 0 && l == 0) hipLaunchKernelGGL(gp::sparse_factor_kernel<256>, dim3(count), dim3(256), 0, s->stream, s->view, first);
    // separator chains through the LDS-staged kernel (the per-entry gather for them as well: 1.45 vs 0.93 ms, profiles/r03_solver_time.txt)
    if (count > 0 && l > 0) hipLaunchKernelGGL(gp::sparse_factor_staged_kernel<1024>, dim3(count), dim3(1024), 0, s->stream, s->view, first);
  }
  for (int l = levels - 1; l >= 0; l--) {
    const int first = S.level_ptr[l], count = S.level_ptr[l + 1] - first;
    if (count > 0) hipLaunchKernelGGL(gp::sparse_backsolve_kernel, dim3(count), dim3(64), 0, s->stream, s->view, first);
  }
}

// SparseLinearSolver::solve(A, b): A x = b by block-sparse LL^T.  The assembled blocks are overwritten by the factor (build again
// before the next solve).  x in slot order.
int gp_sparse_system_solve(gp_sparse_system_t* s, double* x_host, double* x_dev_out) {
  if (!s || !s->built) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_solve: build the system first");
  const gp::SparseSymbolic& S = s->sym;
  GP_HIP(hipMemsetAsync(s->status.ptr, 0, sizeof(int), s->stream));
  launch_factor_and_substitutions(s);
  hipLaunchKernelGGL(gp::sparse_unpermute_kernel, dim3((s->n + 255) / 256), dim3(256), 0, s->stream, (const double*)s->x.as<double>(), s->d_perm, S.P, s->x_slots.as<double>());
  GP_HIP(hipGetLastError());
  s->built = false;
  int h_status = 0;
  GP_HIP(hipMemcpyAsync(&h_status, s->status.ptr, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  if (x_dev_out) GP_HIP(hipMemcpyAsync(x_dev_out, s->x_slots.ptr, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToDevice, s->stream));
  if (x_host) GP_HIP(hipMemcpyAsync(x_host, s->x_slots.ptr, sizeof(double) * (size_t)s->n, hipMemcpyDeviceToHost, s->stream));
  GP_HIP(hipStreamSynchronize(s->stream));
  if (h_status != 0) return gp::fail(GP_ERROR_INDETERMINATE, "gp_sparse_system_solve: the system is not positive definite (indeterminate linear system)");
  return GP_OK;
}

// One damped step of the optimizer's inner loop in ONE stream-ordered pass and ONE synchronisation: buildDampedSystem + solve (levenberg_marquardt_ext.cpp:146-161, 200-220),
// i.e. gp_sparse_system_build, gp_sparse_system_download(b, c) and gp_sparse_system_solve without the two waits and the four copies between them.  2 + 2 x levels launches:
// the assembly (damping applied as the diagonal is written; b, c stored where the host reads them; status cleared), the levels, x (slot order) + status to the host.
// Bit-identical to the three calls.  b_host / c_host are valid also when the system turns out indeterminate (the optimizer raises lambda and tries again).
// the step's device work, queued on the system's stream: nothing waits here
int gp_sparse_system::issue_step(const gp_linearized6* records_dev, const gp::Damping& damping, const double* prior_diag_host, const gp::LmPoseView* epi, bool* fused) {
  if (fused) *fused = epi && one_launch;
  if ((!records_dev && num_factors > 0) || !(damping.lambda >= 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system_step: bad arguments");
  // (a step in flight also owns prior_staged, the source of its pending H2D copy)
  GP_TRY(step.begin(api, (size_t)this->n));
  const gp::SparseSymbolic& S = sym;
  const size_t n = (size_t)this->n;
  double* h = step.host();
  gp::SparseStepExtras ex{};
  ex.lambda = damping.lambda, ex.min_diag = damping.min_diag, ex.max_diag = damping.max_diag, ex.diagonal = damping.diagonal;
  if (prior_diag_host) {
    GP_TRY(upload_prior(this, prior_diag_host, &prior_staged));
    ex.prior_diag = prior.as<double>();
  }
  ex.perm = d_perm, ex.b_slots_host = h + n, ex.c_dev = c.as<double>(), ex.c_host = h + 2 * n, ex.status = status.as<int>();
  ex.num_factors = num_factors, ex.num_dests = (int)dests.size();
  ex.diag0 = diag0.as<double>();
  hipLaunchKernelGGL(gp::sparse_assemble_kernel<true>, dim3((unsigned)dests.size() + 1), dim3(64), 0, stream, d_dests.as<gp::SparseDest>(),
                     d_contribs.as<gp::Contribution>(), reinterpret_cast<const double*>(records_dev), L.as<double>(), y.as<double>(), ex);
  if (one_launch) {
    // small graph: the assembly as it is (one workgroup per block of L across the chip: a gather of 8-byte values, which ONE compute unit's vector memory path takes
    // 40 us for), then factorisation and both substitutions in ONE launch with every operand in the LDS of one compute unit (sparse_small_step_kernel)
    gp::SparseSmallView V = small;
    V.x_slots_host = h;
    V.status_host = h + 2 * n + 1;
    V.has_epi = epi ? 1 : 0;
    if (epi) V.epi = *epi;
    gp::launch_small_step(V, small_lds_bytes, stream, status.as<int>());
  } else {
    launch_factor_and_substitutions(this);
    hipLaunchKernelGGL(gp::sparse_step_end_kernel, dim3((this->n + 255) / 256), dim3(256), 0, stream, (const double*)x.as<double>(), d_perm, S.P, x_slots.as<double>(), h,
                       (const int*)status.as<int>(), h + 2 * n + 1);
  }
  GP_HIP(hipGetLastError());
  built = false;
  step.in_flight = true;
  return GP_OK;
}

// gp_sparse_system_issue_step / _finish_step (waits for the stream and hands over what the step's kernels left in the pinned buffer) / _collect_step (for a caller
// that has SEEN the stream pass the step: no wait of its own) / _step / _set_one_launch / _device_solution
GP_DAMPED_SYSTEM_STEP_API(gp_sparse_system, gp_sparse_system_t)

}  // extern "C"
