// gp_lm_groups.hpp -- how the device-resident LM graph (gp_lm.hip) lays out its variables and records: which pose gets which slot, the (target, source) slots of every
// record, and where each factor family's records start.  The pairwise families are a TABLE of kLmGroups groups, walked in order wherever the graph names them; the
// pose factors' records follow the last group's.  Host code on the standard library and the C header alone -- no HIP header -- so that a host compiler builds it by
// itself (tests/lm_groups_cases.cpp, run under the sanitizers by tests/test_lm_groups_cpu.py).
#pragma once
#include <cstddef>
#include <string>
#include <vector>

#include "../../include/gtsam_points_hip.h"

namespace gp {

constexpr int kLmGroups = 2;
enum : int { kLmVgicp = 0, kLmCorr = 1 };  // record order: the VGICP batch's factors, then the GICP / ICP batch's (gp_corr_batch.hip)
constexpr const char* kLmPairsName[kLmGroups] = {"pose_pairs", "corr_pairs"};

struct LmLayout {
  std::vector<int> slot;                  // [N] variable slot of a pose, -1 = held
  int slots = 0;
  std::vector<int> factor_slots;          // [R][2] (target slot, source slot) per record; a prior is the unary record (-1, slot)
  int record_offset[kLmGroups + 1] = {};  // group k's records are [record_offset[k], record_offset[k] + count[k]); [kLmGroups]: the pose factors'
  int num_records = 0;                    // R
};

// The layout of a graph of count[k] pairwise factors per group over pairs[k] = [count[k]][2] (target pose, source pose), P pose factors (checked by
// gp::check_pose_factors before) and num_poses poses of which pose_fixed (may be null) holds some.  Returns the refusal -- a pair that is not two different poses in
// [0, num_poses), in group order, then a graph whose every pose is held -- or an empty string.
inline std::string lm_layout(const int* const pairs[kLmGroups], const int count[kLmGroups], const gp_pose_factor* pose_factors, int P, int num_poses,
                             const unsigned char* pose_fixed, LmLayout* out) {
  LmLayout& L = *out;
  L = LmLayout{};
  L.slot.assign((size_t)num_poses, -1);
  for (int i = 0; i < num_poses; i++)
    if (!pose_fixed || !pose_fixed[i]) L.slot[(size_t)i] = L.slots++;
  for (int k = 0; k < kLmGroups; k++) {
    L.record_offset[k] = L.num_records;
    L.num_records += count[k];
  }
  L.record_offset[kLmGroups] = L.num_records;
  L.num_records += P;
  L.factor_slots.assign(2 * (size_t)L.num_records, -1);
  for (int k = 0; k < kLmGroups; k++)
    for (int f = 0; f < count[k]; f++) {
      const int t = pairs[k][2 * (size_t)f], s = pairs[k][2 * (size_t)f + 1];
      if (t < 0 || t >= num_poses || s < 0 || s >= num_poses || t == s) return std::string(kLmPairsName[k]) + " entries must be two different poses in [0, num_poses)";
      int* fs = L.factor_slots.data() + 2 * ((size_t)L.record_offset[k] + f);
      fs[0] = L.slot[(size_t)t], fs[1] = L.slot[(size_t)s];
    }
  for (int p = 0; p < P; p++) {  // between: (slot[a], slot[b]); prior: (-1, slot[a])
    const gp_pose_factor& pf = pose_factors[p];
    int* fs = L.factor_slots.data() + 2 * ((size_t)L.record_offset[kLmGroups] + p);
    if (pf.kind == GP_POSE_FACTOR_BETWEEN) fs[0] = L.slot[(size_t)pf.pose_a], fs[1] = L.slot[(size_t)pf.pose_b];
    else fs[1] = L.slot[(size_t)pf.pose_a];
  }
  if (L.slots == 0) return "every pose is held";
  return std::string();
}

}  // namespace gp
