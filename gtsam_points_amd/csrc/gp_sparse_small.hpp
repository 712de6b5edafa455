// gp_sparse_small.hpp -- what gp_sparse.hip hands the one-launch step of small graphs (gp_sparse_small.hip)
#pragma once
#include <hip/hip_runtime.h>

#include "gp_lm_poses.hpp"
#include "gp_sparse_small_lds.hpp"

namespace gp {

enum class SmallForm { LockStep, Teams, LoneWaves };  // how the step walks a level's work lists (gp_sparse_small.hip, phase 1; gp_sparse_system_set_one_launch: 2, 1, 3)

struct SparseSmallView {
  const double* L_global;      // [nnzL][36] column-major: the assembled (damped) blocks
  const double* y_global;      // [6 P] b, elimination order
  const double* diag0_global;  // [6 P] the assembled diagonal
  const int* arena;       // global copy of the index lists below, `arena_words` ints, copied to LDS first
  const int* level_ptr;   // [num_levels + 1] -> work lists (global; read once per level)
  int arena_words, num_levels, P, nnzL;
  // where the lists start (ints) inside the arena, in the order of SmallLists' members (gp_sparse_small.hip): colptr, rowidx, upd_ptr, upd_a, upd_b, row_ptr, row_blk,
  // row_col, work_ptr, work_cols, blkcol (block -> its column), list_maxnb (work list -> the most blocks a column of it has)
  int off[12];
  const int* perm;        // elimination order -> slot (global)
  double* x_slots;        // device, slot order
  double* x_slots_host;   // pinned
  double* status_host;    // pinned
  LmPoseView epi;             // has_epi: the retract of the device-resident LM trial as the kernel's epilogue (gp_lm_poses.hpp)
  int has_epi;
  SmallForm form;
  unsigned long long* trace;  // measurement (gp_debug_sparse_step_trace): shader-clock stamps of thread 0 -- [0] start, [1] = [5] lists and system in LDS, [2] factored, [3] substituted, [4] end,
                              // [8 + 4 r + {0, 1, 2, 3}]: round r < 14 of the first level: start, gathered, diagonal done, blocks below done; null = off
};

bool small_step_available();  // the runtime grants the kernel its dynamic LDS (asked once per system)
void launch_small_step(const SparseSmallView& V, size_t lds_bytes, hipStream_t stream, int* status);  // one 512-thread workgroup on `stream`

}  // namespace gp
