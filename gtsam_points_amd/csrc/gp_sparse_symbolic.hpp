// gp_sparse_symbolic.hpp -- the symbolic phase of the block-sparse solver (gp_sparse_symbolic.hip: pure host code, once per graph)
#pragma once
#include <cstddef>
#include <vector>

namespace gp {

struct SparseSymbolic {
  int P = 0;
  std::vector<int> perm, iperm;    // perm[k] = slot eliminated k-th; iperm[slot] = k
  std::vector<int> parent;         // elimination tree (-1: root)
  std::vector<int> colptr;         // [P + 1] block offsets; column k = its diagonal block followed by its sub-diagonal blocks
  std::vector<int> rowidx;         // [nnzL] row (elimination index) of every block
  std::vector<int> upd_ptr;        // [nnzL + 1] -> upd_a / upd_b: block (i, k) -= L[upd_a] * L[upd_b]^T, in ascending source column
  std::vector<int> upd_a, upd_b;
  std::vector<int> upd_bpos;       // position of block upd_b[u] in the row list of its row k (row_ptr[k] + upd_bpos[u] -> row_blk): the separator kernel stages row k in LDS
  std::vector<int> row_ptr;        // [P + 1] -> row_blk / row_col: the blocks L_kj (j < k) of row k and their columns, ascending j
  std::vector<int> row_blk, row_col;
  std::vector<int> work_ptr, work_cols;  // work lists: [num_subtrees] subtrees, then the CHAINS of the top part (separator columns), grouped by level
  std::vector<int> level_ptr;            // [num_levels + 1] -> work lists: level 0 = the subtrees, level l >= 1 = the top chains whose children are all in lower levels
  int num_subtrees = 0;
  long long nnzA = 0;
};

// ordering: 0 = natural, 1 = nested dissection, 2 = minimum degree, 3 = minimum degree with slack, 4 = automatic
int sparse_symbolic(int num_slots, const int* factor_slots, int num_factors, int ordering, SparseSymbolic* out);
// what one solve walks sequentially: the sum over the levels of the longest work list of the level
int critical_columns(const SparseSymbolic& S);

// LDS bytes the one-launch step of small graphs needs for a symbolic factorisation (small_lds_layout, gp_sparse_small_lds.hpp; 0: the factor does not qualify);
// arena_words_out: the ints of its index lists
size_t small_step_lds_bytes(const SparseSymbolic& S, size_t* arena_words_out = nullptr);

}  // namespace gp
