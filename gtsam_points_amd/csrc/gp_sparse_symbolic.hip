// gp_sparse_symbolic.hip -- the symbolic phase of the block-sparse solver (gp_sparse.hip): pure host code, no kernel and no device call; its entry points are also
// what the CPU tests call.  Once per graph: elimination order (the slot order of the factor key list, nested dissection by BFS bisection of the pose graph, or minimum
// degree), symbolic factorisation (elimination tree, block structure of L incl. fill), for every block of L the ordered list of block products that update it, and the
// level schedule of the numeric phase.
#include <algorithm>
#include <cstring>
#include <functional>
#include <iterator>
#include <numeric>
#include <queue>
#include <vector>

#include "gp_host.hpp"
#include "gp_sparse_small_lds.hpp"
#include "gp_sparse_symbolic.hpp"

namespace gp {

// nested dissection by BFS bisection: order = nd(A) ++ nd(B) ++ separator
static void nested_dissection(const std::vector<std::vector<int>>& adj, std::vector<int>* order) {
  const int P = (int)adj.size();
  std::vector<int> label(P, 0), level(P, -1);  // label: id of the current piece a node belongs to
  order->clear();
  order->reserve(P);
  int next_label = 1;
  std::function<void(const std::vector<int>&)> rec = [&](const std::vector<int>& nodes) {
    if (nodes.size() <= 8) {
      for (int v : nodes) order->push_back(v);
      return;
    }
    const int mine = next_label++;
    for (int v : nodes) label[v] = mine;
    // connected components of the piece
    std::vector<std::vector<int>> comps;
    for (int v : nodes) level[v] = -1;
    for (int s : nodes) {
      if (level[s] != -1) continue;
      comps.emplace_back();
      std::vector<int>& c = comps.back();
      level[s] = 0;
      c.push_back(s);
      for (size_t h = 0; h < c.size(); h++)
        for (int w : adj[c[h]])
          if (label[w] == mine && level[w] == -1) {
            level[w] = 0;
            c.push_back(w);
          }
    }
    if (comps.size() > 1) {
      for (auto& c : comps) {
        std::sort(c.begin(), c.end());
        rec(c);
      }
      return;
    }
    // one component: BFS from a pseudo-peripheral node (two sweeps), cut at the thinnest level near the middle
    auto bfs = [&](int s, std::vector<int>* seq) {
      for (int v : nodes) level[v] = -1;
      seq->clear();
      level[s] = 0;
      seq->push_back(s);
      for (size_t h = 0; h < seq->size(); h++)
        for (int w : adj[(*seq)[h]])
          if (label[w] == mine && level[w] == -1) {
            level[w] = level[(*seq)[h]] + 1;
            seq->push_back(w);
          }
    };
    std::vector<int> seq;
    bfs(nodes[0], &seq);
    bfs(seq.back(), &seq);
    const int depth = level[seq.back()] + 1;
    if (depth < 3) {  // (nearly) complete piece: no useful separator
      for (int v : nodes) order->push_back(v);
      return;
    }
    std::vector<int> width(depth, 0);
    for (int v : nodes) width[level[v]]++;
    std::vector<long long> below(depth + 1, 0);
    for (int l = 0; l < depth; l++) below[l + 1] = below[l] + width[l];
    int cut = -1;
    double best = 1e300;
    for (int l = 1; l + 1 < depth; l++) {
      const double a = (double)below[l], b = (double)(below[depth] - below[l + 1]);
      if (a < 0.25 * nodes.size() || b < 0.25 * nodes.size()) continue;  // balanced enough
      const double score = width[l] + 0.01 * std::abs(a - b);
      if (score < best) {
        best = score;
        cut = l;
      }
    }
    if (cut < 0) cut = depth / 2;
    if (4 * (size_t)width[cut] > nodes.size()) {
      // the separator would be a quarter of the piece or more (band-like pieces a few separators wide): dissecting further only
      // moves columns into the sequential top part.  The piece is eliminated in BFS order instead (a band ordering: low fill).
      for (int v : seq) order->push_back(v);
      return;
    }
    std::vector<int> A, B, S;
    for (int v : nodes) (level[v] < cut ? A : (level[v] > cut ? B : S)).push_back(v);
    rec(A);
    rec(B);
    for (int v : S) order->push_back(v);
  };
  std::vector<int> all(P);
  std::iota(all.begin(), all.end(), 0);
  rec(all);
}

// minimum degree by multiple elimination (ordering = 2): every round eliminates an independent set of the nodes whose degree in the current
// elimination graph is within `slack` of the minimum -- the fill-reducing heuristic of GTSAM's default COLAMD-class orderings (which is what
// the reference's solves run with, optimizers/levenberg_marquardt_ext.cpp:200-220), in its multiple-elimination form because independent nodes
// of one round are siblings in the elimination tree: the rounds are what the device schedule runs side by side.  slack = 0 is the classical
// MMD; slack = 1 lets e.g. the interior nodes of a chain (degree 2, against 1 at the two ends) go in the first round, which makes a chain's
// tree logarithmic instead of one path.  Deterministic: ties by node index.  The graph is explicit (sorted neighbour lists incl. fill), fine
// for pose graphs of 10^4 nodes.
static void minimum_degree(const std::vector<std::vector<int>>& adj0, int slack, std::vector<int>* order) {
  const int P = (int)adj0.size();
  std::vector<std::vector<int>> adj = adj0;
  std::vector<char> gone((size_t)P, 0), blocked((size_t)P, 0);
  order->clear();
  order->reserve(P);
  std::vector<int> cand, merged;
  int left = P;
  while (left > 0) {
    int dmin = P + 1;
    for (int v = 0; v < P; v++)
      if (!gone[v]) dmin = std::min(dmin, (int)adj[v].size());
    cand.clear();
    for (int v = 0; v < P; v++)
      if (!gone[v] && (int)adj[v].size() <= dmin + slack) cand.push_back(v);
    std::stable_sort(cand.begin(), cand.end(), [&](int a, int b) { return adj[a].size() < adj[b].size(); });
    std::fill(blocked.begin(), blocked.end(), 0);
    for (int v : cand) {
      if (blocked[v]) continue;
      // eliminate v: its neighbours become a clique
      const std::vector<int> nb = adj[v];
      for (int a : nb) {
        blocked[a] = 1;  // not in this round: its degree has just changed
        merged.clear();
        std::set_union(adj[a].begin(), adj[a].end(), nb.begin(), nb.end(), std::back_inserter(merged));
        merged.erase(std::remove_if(merged.begin(), merged.end(), [&](int w) { return w == a || w == v; }), merged.end());
        adj[a].swap(merged);
      }
      adj[v].clear();
      gone[v] = 1;
      left--;
      order->push_back(v);
    }
  }
}

static int sparse_symbolic_with(int num_slots, const int* factor_slots, int num_factors, int ordering, SparseSymbolic* out) {
  SparseSymbolic& S = *out;
  const int P = num_slots;
  S.P = P;
  // pose graph
  std::vector<std::vector<int>> adj((size_t)P);
  for (int f = 0; f < num_factors; f++) {
    const int a = factor_slots[2 * f], b = factor_slots[2 * f + 1];
    if (a >= P || b >= P) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system: slot index out of range");
    if (a >= 0 && a == b) return fail(GP_ERROR_INVALID_ARGUMENT, "gp_sparse_system: a factor needs two different poses");
    if (a >= 0 && b >= 0) {
      adj[a].push_back(b);
      adj[b].push_back(a);
    }
  }
  for (auto& v : adj) {
    std::sort(v.begin(), v.end());
    v.erase(std::unique(v.begin(), v.end()), v.end());
  }
  S.perm.resize(P);
  if (ordering == 1) {
    nested_dissection(adj, &S.perm);
  } else if (ordering == 2 || ordering == 3) {
    minimum_degree(adj, ordering == 2 ? 0 : 1, &S.perm);
  } else {
    std::iota(S.perm.begin(), S.perm.end(), 0);
  }
  S.iperm.assign(P, -1);
  for (int k = 0; k < P; k++) S.iperm[S.perm[k]] = k;
  // structure of A below the diagonal, per column, in elimination indices
  std::vector<std::vector<int>> col((size_t)P);
  S.nnzA = P;
  for (int v = 0; v < P; v++)
    for (int w : adj[v]) {
      const int i = S.iperm[v], j = S.iperm[w];
      if (i > j) {
        col[j].push_back(i);
        S.nnzA++;
      }
    }
  // symbolic Cholesky: struct(L_j) = struct(A_j) U (struct(L_c) \ {j}) over the children c of j in the elimination tree
  S.parent.assign(P, -1);
  std::vector<std::vector<int>> children((size_t)P);
  for (int j = 0; j < P; j++) {
    std::vector<int>& s = col[j];
    for (int c : children[j])
      for (int r : col[c])
        if (r != j) s.push_back(r);
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    if (!s.empty()) {
      S.parent[j] = s[0];
      children[s[0]].push_back(j);
    }
  }
  S.colptr.assign(P + 1, 0);
  for (int j = 0; j < P; j++) S.colptr[j + 1] = S.colptr[j] + 1 + (int)col[j].size();
  const int nnzL = S.colptr[P];
  S.rowidx.resize(nnzL);
  for (int j = 0; j < P; j++) {
    S.rowidx[S.colptr[j]] = j;
    for (size_t q = 0; q < col[j].size(); q++) S.rowidx[S.colptr[j] + 1 + q] = col[j][q];
  }
  auto find_block = [&](int i, int k) {  // block (i, k), i >= k, must exist
    if (i == k) return S.colptr[k];
    const auto it = std::lower_bound(col[k].begin(), col[k].end(), i);
    return S.colptr[k] + 1 + (int)(it - col[k].begin());
  };
  // update lists (two passes: count, fill), source columns in ascending order; row lists for the substitutions
  S.upd_ptr.assign(nnzL + 1, 0);
  S.row_ptr.assign(P + 1, 0);
  for (int j = 0; j < P; j++)
    for (size_t q = 0; q < col[j].size(); q++) {
      const int k = col[j][q];
      S.row_ptr[k + 1]++;
      for (size_t p = q; p < col[j].size(); p++) S.upd_ptr[find_block(col[j][p], k) + 1]++;
    }
  for (int d = 0; d < nnzL; d++) S.upd_ptr[d + 1] += S.upd_ptr[d];
  for (int k = 0; k < P; k++) S.row_ptr[k + 1] += S.row_ptr[k];
  S.upd_a.resize(S.upd_ptr[nnzL]);
  S.upd_b.resize(S.upd_ptr[nnzL]);
  S.upd_bpos.resize(S.upd_ptr[nnzL]);
  S.row_blk.resize(S.row_ptr[P]);
  S.row_col.resize(S.row_ptr[P]);
  {
    std::vector<int> ucur(S.upd_ptr.begin(), S.upd_ptr.end() - 1), rcur(S.row_ptr.begin(), S.row_ptr.end() - 1);
    for (int j = 0; j < P; j++)
      for (size_t q = 0; q < col[j].size(); q++) {
        const int k = col[j][q], bkj = S.colptr[j] + 1 + (int)q;
        S.row_blk[rcur[k]] = bkj;
        S.row_col[rcur[k]++] = j;
        for (size_t p = q; p < col[j].size(); p++) {
          const int d = find_block(col[j][p], k);
          S.upd_a[ucur[d]] = S.colptr[j] + 1 + (int)p;
          S.upd_bpos[ucur[d]] = rcur[k] - 1 - S.row_ptr[k];
          S.upd_b[ucur[d]++] = bkj;
        }
      }
  }
  // schedule: cut the elimination forest into independent subtrees + the top
  std::vector<long long> weight((size_t)P, 0);
  for (int j = 0; j < P; j++) {
    const long long nb = 1 + (long long)col[j].size();
    weight[j] += nb * nb;  // ~ block products + solves of the column
    if (S.parent[j] >= 0) weight[S.parent[j]] += weight[j];
  }
  std::vector<char> in_top((size_t)P, 0);
  std::priority_queue<std::pair<long long, int>> heap;
  for (int j = 0; j < P; j++)
    if (S.parent[j] < 0) heap.push({weight[j], j});
  // the heaviest subtree is split at its first branching column: the path from its root down to that column goes to the top, the
  // branches become subtrees of their own.  A subtree that is one path down to a leaf cannot be split (nothing in it runs in parallel).
  const size_t want = 256;
  std::vector<int> roots;
  while (!heap.empty() && heap.size() + roots.size() < want) {
    const int r = heap.top().second;
    heap.pop();
    int b = r;
    while (children[b].size() == 1) b = children[b][0];
    if (children[b].empty()) {
      roots.push_back(r);
      continue;
    }
    for (int v = r;; v = children[v][0]) {
      in_top[v] = 1;
      if (v == b) break;
    }
    for (int c : children[b]) heap.push({weight[c], c});
  }
  std::vector<int> owner((size_t)P, -1);  // subtree id; -1: top
  S.num_subtrees = 0;
  while (!heap.empty()) {
    roots.push_back(heap.top().second);
    heap.pop();
  }
  std::sort(roots.begin(), roots.end());
  for (int r : roots) owner[r] = S.num_subtrees++;
  for (int j = P - 1; j >= 0; j--)
    if (!in_top[j] && owner[j] < 0) owner[j] = owner[S.parent[j]];  // parent index > child index: the parent is done
  // the top part, level-scheduled: its columns are cut into CHAINS (a column with exactly one child in the top continues that child's chain)
  // and a chain's level is one above the highest level among the chains below it (subtrees: level 0).  One launch per level, one workgroup
  // per chain: the separators of a dissection's level l run side by side instead of behind each other on one workgroup (round 2: band graphs
  // spent 4-5 ms there).
  std::vector<int> chain_of((size_t)P, -1), chain_level;
  std::vector<std::vector<int>> chain_cols;
  for (int j = 0; j < P; j++) {  // children precede parents
    if (!in_top[j]) continue;
    int top_children = 0, only = -1, lvl = 1;
    for (int c : children[j]) {
      if (in_top[c]) {
        top_children++;
        only = c;
        lvl = std::max(lvl, chain_level[(size_t)chain_of[c]] + 1);
      }
    }
    if (top_children == 1) {
      chain_of[j] = chain_of[only];
      chain_cols[(size_t)chain_of[j]].push_back(j);
    } else {
      chain_of[j] = (int)chain_cols.size();
      chain_cols.push_back({j});
      chain_level.push_back(lvl);
    }
  }
  int num_levels = 1;
  for (int l : chain_level) num_levels = std::max(num_levels, l + 1);
  std::vector<std::vector<int>> by_level((size_t)num_levels);
  for (size_t c = 0; c < chain_cols.size(); c++) by_level[(size_t)chain_level[c]].push_back((int)c);
  const int num_lists = S.num_subtrees + (int)chain_cols.size();
  S.work_ptr.assign(num_lists + 1, 0);
  S.work_cols.clear();
  S.work_cols.reserve(P);
  S.level_ptr.assign(1, 0);
  {
    std::vector<std::vector<int>> sub((size_t)S.num_subtrees);
    for (int j = 0; j < P; j++)
      if (!in_top[j]) sub[(size_t)owner[j]].push_back(j);  // ascending inside every list
    int list = 0;
    for (auto& cols : sub) {
      S.work_cols.insert(S.work_cols.end(), cols.begin(), cols.end());
      S.work_ptr[++list] = (int)S.work_cols.size();
    }
    S.level_ptr.push_back(list);
    for (int l = 1; l < num_levels; l++) {
      for (int c : by_level[(size_t)l]) {
        S.work_cols.insert(S.work_cols.end(), chain_cols[(size_t)c].begin(), chain_cols[(size_t)c].end());
        S.work_ptr[++list] = (int)S.work_cols.size();
      }
      S.level_ptr.push_back(list);
    }
  }
  return GP_OK;
}

// what one solve walks sequentially: the sum over the levels of the longest work list of the level
int critical_columns(const SparseSymbolic& S) {
  int crit = 0;
  for (size_t l = 0; l + 1 < S.level_ptr.size(); l++) {
    int longest = 0;
    for (int w = S.level_ptr[l]; w < S.level_ptr[l + 1]; w++) longest = std::max(longest, S.work_ptr[w + 1] - S.work_ptr[w]);
    crit += longest;
  }
  return crit;
}

// LDS bytes the one-launch step needs for a symbolic factorisation: L's blocks, y, x, the teams' scratch, the index lists
size_t small_step_lds_bytes(const SparseSymbolic& S, size_t* arena_words_out) {
  const size_t words = S.colptr.size() + S.rowidx.size() + S.upd_ptr.size() + S.upd_a.size() + S.upd_b.size() + S.row_ptr.size() + S.row_blk.size() + S.row_col.size() +
                       S.work_ptr.size() + S.work_cols.size() + S.rowidx.size() /* the blocks' columns */ + S.work_ptr.size() /* the lists' widest columns */ + 2;
  if (arena_words_out) *arena_words_out = words;
  if (S.P > 128) return 0;  // (row lists stay below the staged kernel's 128-block stage, which the one-launch form assumes)
  const size_t bytes = small_lds_layout((size_t)S.P, (size_t)S.colptr[S.P], words).bytes;
  return bytes <= kSmallLdsCeiling ? bytes : 0;
}
static bool small_step_fits(const SparseSymbolic& S) { return small_step_lds_bytes(S) != 0; }

// ordering = 4 (automatic): nested dissection and minimum degree with slack are both tried and the schedule with the shorter critical path
// (then the smaller factor) is kept -- band-like graphs want the dissection (separators side by side), graphs with random loop closures and
// grids the minimum degree (less fill AND a shorter path); the symbolic phase is host code run once per graph
int sparse_symbolic(int num_slots, const int* factor_slots, int num_factors, int ordering, SparseSymbolic* out) {
  if (ordering != 4) return sparse_symbolic_with(num_slots, factor_slots, num_factors, ordering, out);
  SparseSymbolic a, b;
  GP_TRY(sparse_symbolic_with(num_slots, factor_slots, num_factors, 1, &a));
  GP_TRY(sparse_symbolic_with(num_slots, factor_slots, num_factors, 3, &b));
  const int ca = critical_columns(a), cb = critical_columns(b);
  bool take_b = cb < ca || (cb == ca && b.colptr[num_slots] < a.colptr[num_slots]);
  // round 6: a factor that fits one compute unit's LDS is solved by ONE launch with every operand in LDS (sparse_small_step_kernel: ~2 us per column instead of 6-8), which
  // outweighs a shorter critical path in columns -- BASELINE configs[2]'s graph: dissection 21 columns / 522 blocks (150 KB: does not fit), minimum degree 34 columns /
  // 305 blocks (fits).  Between two that qualify, or two that do not, the rule above stands.
  const bool fa = small_step_fits(a), fb = small_step_fits(b);
  if (fa != fb) take_b = fb;
  *out = take_b ? std::move(b) : std::move(a);
  return GP_OK;
}

// the argument check of the entry points below, then the symbolic phase; `what` = the message of a refusal
static int checked_symbolic(int num_slots, const int* factor_slots, int num_factors, int ordering, bool outputs_ok, const char* what, SparseSymbolic* S) {
  if (num_slots <= 0 || num_factors < 0 || (num_factors > 0 && !factor_slots) || ordering < 0 || ordering > 4 || !outputs_ok) return fail(GP_ERROR_INVALID_ARGUMENT, what);
  return sparse_symbolic(num_slots, factor_slots, num_factors, ordering, S);
}

}  // namespace gp

extern "C" {

int gp_sparse_symbolic(int num_slots, const int* factor_slots, int num_factors, int ordering, int* perm_out, int* parent_out, int64_t* nnz_a_blocks, int64_t* nnz_l_blocks,
                       int* num_subtrees, int* top_columns) {
  gp::SparseSymbolic S;
  GP_TRY(gp::checked_symbolic(num_slots, factor_slots, num_factors, ordering, true,
                              "gp_sparse_symbolic: bad arguments (ordering: 0 = natural, 1 = nested dissection, 2 = minimum degree, 3 = minimum degree with slack, 4 = automatic)", &S));
  if (perm_out) memcpy(perm_out, S.perm.data(), sizeof(int) * (size_t)num_slots);
  if (parent_out) memcpy(parent_out, S.parent.data(), sizeof(int) * (size_t)num_slots);
  if (nnz_a_blocks) *nnz_a_blocks = S.nnzA;
  if (nnz_l_blocks) *nnz_l_blocks = S.colptr[num_slots];
  if (num_subtrees) *num_subtrees = S.num_subtrees;
  if (top_columns) *top_columns = num_slots - S.work_ptr[S.num_subtrees];
  return GP_OK;
}

// the schedule of the numeric phase (pure host code): number of launch levels (level 0 = the subtrees) and the critical path in columns, i.e. the
// sum over the levels of the longest work list of the level -- what one solve walks sequentially
int gp_sparse_symbolic_schedule(int num_slots, const int* factor_slots, int num_factors, int ordering, int* num_levels, int* critical_columns, int* num_lists) {
  gp::SparseSymbolic S;
  GP_TRY(gp::checked_symbolic(num_slots, factor_slots, num_factors, ordering, true, "gp_sparse_symbolic_schedule: bad arguments", &S));
  const int levels = (int)S.level_ptr.size() - 1;
  if (num_levels) *num_levels = levels;
  if (critical_columns) *critical_columns = gp::critical_columns(S);
  if (num_lists) *num_lists = S.level_ptr[levels];
  return GP_OK;
}

// host-side check hook (no device needed): the work lists of the numeric phase -- per list its level, its number of columns, the block products its columns gather in
// all and the most a single column gathers; arrays of `capacity` ints (num_lists from gp_sparse_symbolic_schedule)
int gp_debug_sparse_work_lists(int num_slots, const int* factor_slots, int num_factors, int ordering, int capacity, int* level, int* columns, int* products, int* max_column_products) {
  gp::SparseSymbolic S;
  GP_TRY(gp::checked_symbolic(num_slots, factor_slots, num_factors, ordering, level && columns && products && max_column_products, "gp_debug_sparse_work_lists: bad arguments", &S));
  const int levels = (int)S.level_ptr.size() - 1;
  if (S.level_ptr[levels] > capacity) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_debug_sparse_work_lists: capacity too small");
  for (int l = 0; l < levels; l++)
    for (int w = S.level_ptr[l]; w < S.level_ptr[l + 1]; w++) {
      level[w] = l;
      columns[w] = S.work_ptr[w + 1] - S.work_ptr[w];
      int sum = 0, mx = 0;
      for (int q = S.work_ptr[w]; q < S.work_ptr[w + 1]; q++) {
        const int k = S.work_cols[q];
        const int n = S.upd_ptr[S.colptr[k + 1]] - S.upd_ptr[S.colptr[k]];
        sum += n;
        mx = std::max(mx, n);
      }
      products[w] = sum;
      max_column_products[w] = mx;
    }
  return GP_OK;
}

}  // extern "C"
