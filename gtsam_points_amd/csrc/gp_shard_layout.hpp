// gp_shard_layout.hpp -- which factors a shard of the multi-GPU batch (gp_multi.hip) holds and where their rows lie in the [F x width] stack: the balanced contiguous
// plan (gp_shard_plan_*), the layout of ANY assignment of factors to shards (one function: the batch's create on both of its routes and gp_debug_multi_gather_plan
// go through it), and the send offset of the in-place all-gather.  Host arithmetic on the standard library and the C header alone -- no HIP header -- so that a host
// compiler builds it by itself (tests/shard_layout_cases.cpp, run under the sanitizers by tests/test_shard_layout_cpu.py).
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

#include "../../include/gtsam_points_hip.h"

namespace gp {

// contiguous partition of w[0..n) into k ranges minimising the largest range sum (binary search on the bound + greedy fill)
inline std::vector<int> balanced_boundaries(const int64_t* w, int n, int k) {
  std::vector<int> best((size_t)k + 1, n);
  best[0] = 0;
  if (n == 0) return best;
  int64_t lo = 0, hi = 0;
  for (int i = 0; i < n; i++) {
    lo = std::max(lo, w[i]);
    hi += w[i];
  }
  auto fill = [&](int64_t bound, std::vector<int>* out) {
    int shard = 0;
    int64_t acc = 0;
    std::vector<int> b((size_t)k + 1, n);
    b[0] = 0;
    for (int i = 0; i < n; i++) {
      if (acc + w[i] > bound && acc > 0) {
        shard++;
        if (shard >= k) return false;
        b[(size_t)shard] = i;
        acc = 0;
      }
      acc += w[i];
    }
    if (out) *out = b;
    return true;
  };
  while (lo < hi) {
    const int64_t mid = lo + (hi - lo) / 2;
    if (fill(mid, nullptr)) hi = mid;
    else lo = mid + 1;
  }
  fill(lo, &best);
  // the greedy fill may need fewer than k ranges: split the heaviest range that still holds two factors (at the point that
  // balances its halves) until every shard has work or every factor stands alone -- splitting never raises the maximum
  std::vector<int> cuts;  // begins of the non-empty ranges
  for (int s = 0; s < k; s++)
    if (best[(size_t)s] < best[(size_t)s + 1]) cuts.push_back(best[(size_t)s]);
  auto sum = [&](int a, int b) {
    int64_t t = 0;
    for (int i = a; i < b; i++) t += w[i];
    return t;
  };
  while ((int)cuts.size() < std::min(k, n)) {
    int pick = -1;
    int64_t heaviest = -1;
    for (size_t r = 0; r < cuts.size(); r++) {
      const int a = cuts[r], b = r + 1 < cuts.size() ? cuts[r + 1] : n;
      if (b - a >= 2 && sum(a, b) > heaviest) {
        heaviest = sum(a, b);
        pick = (int)r;
      }
    }
    if (pick < 0) break;
    const int a = cuts[(size_t)pick], b = (size_t)pick + 1 < cuts.size() ? cuts[(size_t)pick + 1] : n;
    int at = a + 1;
    int64_t best_max = -1;
    for (int c = a + 1; c < b; c++) {
      const int64_t m = std::max(sum(a, c), sum(c, b));
      if (best_max < 0 || m < best_max) {
        best_max = m;
        at = c;
      }
    }
    cuts.insert(cuts.begin() + pick + 1, at);
  }
  for (int s = 0; s <= k; s++) best[(size_t)s] = s < (int)cuts.size() ? cuts[(size_t)s] : n;
  return best;
}

struct ShardRows {
  std::vector<int> index;  // global indices of this shard's factors, ascending
  bool contiguous = true;  // index is the one range [first_row, first_row + index.size())
  int first_row = 0;       // index[0]; 0 for a shard without factors
};

struct ShardLayout {
  std::vector<ShardRows> shards;
  size_t gather_rows = 0;  // the in-place all-gather applies iff shard k is exactly rows [k * F / N, (k + 1) * F / N): rows per shard, or 0
};

// The layout of the assignment shard_of[0..num_factors) over num_shards > 0 shards.  Returns GP_OK, or GP_ERROR_INVALID_ARGUMENT with *reason (for the caller's
// gp::fail, behind its own name) when an entry is no shard.
inline int shard_layout(const int* shard_of, int num_factors, int num_shards, ShardLayout* out, const char** reason) {
  ShardLayout& L = *out;
  L = ShardLayout{};
  L.shards.resize((size_t)num_shards);
  for (int i = 0; i < num_factors; i++) {
    if (shard_of[i] < 0 || shard_of[i] >= num_shards) {
      *reason = "shard index out of range";
      return GP_ERROR_INVALID_ARGUMENT;
    }
    L.shards[(size_t)shard_of[i]].index.push_back(i);
  }
  const size_t F = (size_t)num_factors, N = (size_t)num_shards;
  L.gather_rows = F > 0 && F % N == 0 ? F / N : 0;
  for (size_t k = 0; k < N; k++) {
    ShardRows& s = L.shards[k];
    s.first_row = s.index.empty() ? 0 : s.index[0];
    for (size_t j = 1; j < s.index.size(); j++)
      if (s.index[j] != s.index[j - 1] + 1) s.contiguous = false;
    if (!s.contiguous || s.index.size() != L.gather_rows || (size_t)s.first_row != k * L.gather_rows) L.gather_rows = 0;
  }
  return GP_OK;
}

// In-place all-gather: a shard's send buffer is where its own rows already lie in the stack, i.e. at its first global factor index (the gather plan makes shard k
// exactly rows [k * rows, (k + 1) * rows)). Derived from the plan, never from where the Shard object lives (the shards sit in a std::deque, whose
// elements are not contiguous -- `&s - &shards[0]` is undefined for every shard but the first).
inline size_t gather_send_offset(const ShardRows& s, int width) { return (size_t)s.first_row * (size_t)width; }

}  // namespace gp
