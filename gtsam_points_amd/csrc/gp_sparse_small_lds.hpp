// gp_sparse_small_lds.hpp -- the launch geometry and the LDS layout of the one-launch step (sparse_small_step_kernel, gp_sparse_small.hip).  The host's budget
// (small_step_lds_bytes: the ordering-4 choice and gp_sparse_system_create) and the kernel's pointers both come from small_lds_layout
#pragma once
#include <cstddef>

namespace gp {

// one 512-thread workgroup (eight waves of up to 256 registers: the wave form's rows live in registers; at 1024 threads the 128-register cap spilled them;
// tests/test_sparse_build_cpu.py holds the kernel to that), up to eight work lists of a level side by side
constexpr int kSmallThreads = 512, kSmallTeams = 8;
constexpr int kSmallTeamDoubles = 158;  // per team: D[6][7] | rhs[6] | v[6] (backward) | pad 2 | part: rpart[16][6] (forward) / bpart[6][6] (backward) | dinv[6]
constexpr size_t kSmallLdsCeiling = 160 * 1024 - 1024;  // dynamic LDS the kernel is allowed to ask for

// where the pieces start, in doubles from the start of the dynamic LDS: L's blocks [nnzL][36] at 0, then y, x, the reciprocals of L's diagonal and the assembled
// diagonal of A (the pivots' scale), [6 P] each, the teams' scratch [kSmallTeams][kSmallTeamDoubles], the index lists (`words` ints); bytes: all of it + 64
struct SmallLdsLayout { size_t ys, xs, dis, d0s, scr, idx, bytes; };
__host__ __device__ inline SmallLdsLayout small_lds_layout(const size_t P, const size_t nnzL, const size_t words) {
  SmallLdsLayout o;
  o.ys = 36 * nnzL;
  o.xs = o.ys + 6 * P;
  o.dis = o.xs + 6 * P;
  o.d0s = o.dis + 6 * P;
  o.scr = o.d0s + 6 * P;
  o.idx = o.scr + (size_t)kSmallTeams * kSmallTeamDoubles;
  o.bytes = sizeof(double) * o.idx + sizeof(int) * words + 64;
  return o;
}

}  // namespace gp
