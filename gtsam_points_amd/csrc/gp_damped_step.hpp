// gp_damped_step.hpp -- the pieces of the damped step that the dense system (gp_solver.hip) and the block-sparse system (gp_sparse.hip, gp_sparse_multi.hpp, gp_sparse_small.hip) share: the gather of A and b
// out of the factors' gp_linearized6 records, the error sum, the damping, the pivot rule, the host-side contribution lists (the pinned step hand-off and the seam the
// two systems share towards their callers are gp_host.hpp's: StepHandoff, DampedSystem).  Both
// systems call THESE, so a change to the step is made once and the two cannot drift apart.
#pragma once
#include <cstring>
#include <map>
#include <string>
#include <vector>

#include "gp_host.hpp"

namespace gp {

// ---- the records ----------------------------------------------------------------------------------------------------------------------------------------------------

constexpr int REC_HT = 2, REC_HS = 38, REC_HTS = 74, REC_BT = 110, REC_BS = 116;  // offsets (doubles) inside gp_linearized6

// which 6x6 of a record a contribution takes: H_target, H_source, H_target_source (as is: row = target, col = source) or
// its transpose (row = source, col = target)
enum : int { TAKE_HT = 0, TAKE_HS = 1, TAKE_HTS = 2, TAKE_HTS_T = 3 };

struct Contribution {
  int factor;
  int take;
};

// entry (r, c) of a destination block: its contributions summed in list order
__device__ __forceinline__ double gather_h(const Contribution* __restrict__ contribs, int begin, int count, const double* __restrict__ records, int r, int c) {
  double s = 0.0;
  for (int k = 0; k < count; k++) {
    const Contribution q = contribs[begin + k];
    const double* rec = records + 122 * (size_t)q.factor;
    double v;
    if (q.take == TAKE_HT) {
      v = rec[REC_HT + c * 6 + r];
    } else if (q.take == TAKE_HS) {
      v = rec[REC_HS + c * 6 + r];
    } else if (q.take == TAKE_HTS) {
      v = rec[REC_HTS + c * 6 + r];
    } else {
      v = rec[REC_HTS + r * 6 + c];
    }
    s += v;
  }
  return s;
}

// entry r of b at a diagonal destination: the sum of g = -b_target / -b_source (HessianFactor(.., -b_t, .., -b_s, ..), integrated_matching_cost_factor.cpp:49)
__device__ __forceinline__ double gather_g(const Contribution* __restrict__ contribs, int begin, int count, const double* __restrict__ records, int r) {
  double s = 0.0;
  for (int k = 0; k < count; k++) {
    const Contribution q = contribs[begin + k];
    const double* rec = records + 122 * (size_t)q.factor;
    s -= q.take == TAKE_HT ? rec[REC_BT + r] : rec[REC_BS + r];
  }
  return s;
}

// c = the sum of the factors' errors (record word 1) in one fixed order: 256 strided partial sums (partial i adds factors i, i + 256, ...), folded pairwise,
// part[i] += part[i + w] for w = 128 .. 1.  Every thread of a workgroup of NT = 256 threads or 64 lanes calls (a lane then carries partials t, t + 64, t + 128,
// t + 192); the sum is returned to all of them.
template <int NT>
__device__ __forceinline__ double sum_errors(const double* __restrict__ records, int num_factors) {
  __shared__ double part[256];
  const int t = threadIdx.x;
  for (int q = 0; q < 256 / NT; q++) {
    double s = 0.0;
    for (int f = t + NT * q; f < num_factors; f += 256) s += records[122 * (size_t)f + 1];
    part[t + NT * q] = s;
  }
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    for (int i = t; i < w; i += NT) part[i] += part[i + w];
    __syncthreads();
  }
  return part[0];
}

// the error sum of gp_*_system_build
template <int UNUSED = 0>
__global__ void __launch_bounds__(256) sum_errors_kernel(const double* __restrict__ records, int num_factors, double* __restrict__ c_out) {
  const double c = sum_errors<256>(records, num_factors);
  if (threadIdx.x == 0) *c_out = c;
}

// buildDampedSystem (levenberg_marquardt_ext.cpp:146-161): a diagonal entry d of A becomes d + lambda (identity damping) or d + lambda * clamp(d, min, max)
// (diagonalDamping), plus the prior's entry when there is one.  Each operation rounds on its own (no fma contraction), so every caller gets the same bits whether
// or not a branch of its own stands between the multiply and the add.
__device__ __forceinline__ double damped_diagonal(double d, double lambda, int diagonal, double min_diag, double max_diag, const double* prior) {
#pragma clang fp contract(off)
  double add = diagonal ? lambda * fmin(fmax(d, min_diag), max_diag) : lambda;
  if (prior) add += *prior;
  return d + add;
}

// A pivot must exceed kPivotTolerance x the damped assembled diagonal entry of A it came from (the scale), in the dense and the sparse step alike, so that both call
// the same systems indeterminate (include/gtsam_points_hip.h, GP_ERROR_INDETERMINATE).  Asking for piv > 0 left it to rounding whether a SINGULAR system (gauge
// freedom: no pose held) was reported: a pivot of ~1e-13 A_pp came out with either sign, and a positive one solved into a huge step.  GTSAM's own Cholesky treats
// pivots below a threshold as zero (base/cholesky.cpp: zeroPivotThreshold) for the same reason.  1e-11 relative: a system conditioned worse than that has no digits left.
constexpr double kPivotTolerance = 1e-11;
__device__ __forceinline__ bool pivot_ok(double piv, double scale) { return piv > kPivotTolerance * scale; }

// ---- host set-up ----------------------------------------------------------------------------------------------------------------------------------------------------

// The assembly's gather lists: per destination block, the contributions of the factors in factor order (the summation order: no atomics, the same bits every time).
// pos[slot] = the pose's block row / column (the slot itself for the dense system, its elimination index for the sparse one); key(i, j), i >= j = the destination of
// block (i, j); every key in `always` is a destination even without a contribution.  Destinations come out in key order, each as make_dest(key, begin, count).
template <class Key, class Dest, class KeyOf, class MakeDest>
void contribution_lists(const int* factor_slots, int num_factors, const std::vector<int>& pos, const std::vector<Key>& always, KeyOf key, MakeDest make_dest,
                        std::vector<Dest>* dests, std::vector<Contribution>* contribs) {
  std::map<Key, std::vector<Contribution>> lists;
  for (const Key& k : always) lists[k];
  for (int f = 0; f < num_factors; f++) {
    const int st = factor_slots[2 * f], ss = factor_slots[2 * f + 1];
    const int it = st >= 0 ? pos[st] : -1, is = ss >= 0 ? pos[ss] : -1;
    if (it >= 0) lists[key(it, it)].push_back({f, TAKE_HT});
    if (is >= 0) lists[key(is, is)].push_back({f, TAKE_HS});
    if (it >= 0 && is >= 0) {
      if (it > is) {
        lists[key(it, is)].push_back({f, TAKE_HTS});    // row = target, col = source
      } else {
        lists[key(is, it)].push_back({f, TAKE_HTS_T});  // row = source, col = target
      }
    }
  }
  for (auto& kv : lists) {
    dests->push_back(make_dest(kv.first, (int)contribs->size(), (int)kv.second.size()));
    contribs->insert(contribs->end(), kv.second.begin(), kv.second.end());
  }
}

}  // namespace gp
