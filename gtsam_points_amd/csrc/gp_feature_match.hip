// gp_feature_match.hip -- the exact 1-NN search among feature rows, brute force through LDS: gp_feature_nn_search, and through launch_feature_nn
// (gp_feature_match.hpp) the matching of RANSAC (gp_registration.hip; registration/impl/ransac_impl.hpp:62) and of gp_gnc.hip.  The contract is in
// include/gtsam_points_hip.h.  The distances a host restatement has to reproduce to the bit are accumulated by explicit fma() calls: contraction is off for the whole unit.
#pragma clang fp contract(off)

#include <cmath>

#include "gp_feature_match.hpp"

namespace gp {

// One workgroup = kMatchQueries queries (four per wave), every target row.  The target rows pass through LDS in tiles of 64 (row stride dim | 1 words: the lanes of a
// wave read one column of 64 rows without bank conflicts for any dim); lane t of each wave holds target t of the tile against its wave's four queries, so a target
// element read from LDS serves four sums.  Each lane keeps its best (strict <, ascending index: the lowest index among its ties); the wave's 64 are reduced by
// shuffles, equal distances to the lower index.
constexpr int kMatchQueries = 16;
constexpr int kMatchTile = 64;
__global__ __launch_bounds__(256) void feature_nn_kernel(const float* __restrict__ target, int nt, const float* __restrict__ query, int num_rows, int dim,
                                                         const int* __restrict__ rows, int nq, const int* __restrict__ stop, int* __restrict__ out_index,
                                                         double* __restrict__ out_sq_dist) {
  __shared__ float q_lds[kMatchQueries * GP_FEATURE_MAX_DIM];
  __shared__ float t_lds[kMatchTile * (GP_FEATURE_MAX_DIM + 1)];
  if (stop && *stop) return;
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int stride = dim | 1;
  const int q0 = blockIdx.x * kMatchQueries;
  for (int q = wave; q < kMatchQueries; q += 4) {
    const int qi = q0 + q;
    int row = -1;
    if (qi < nq) row = rows ? rows[qi] : qi;
    if (row >= num_rows) row = -1;
    for (int c = lane; c < dim; c += 64) q_lds[q * GP_FEATURE_MAX_DIM + c] = row >= 0 ? query[(size_t)row * dim + c] : __builtin_nanf("");
  }
  double best[4];
  int best_i[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {
    best[k] = INFINITY;
    best_i[k] = -1;
  }
  for (int t0 = 0; t0 < nt; t0 += kMatchTile) {
    __syncthreads();  // the queries are in; the previous tile has been read
    const int rows_here = min(kMatchTile, nt - t0);
    for (int r = wave; r < rows_here; r += 4)
      for (int c = lane; c < dim; c += 64) t_lds[r * stride + c] = target[(size_t)(t0 + r) * dim + c];
    __syncthreads();
    if (lane < rows_here) {
      double acc0 = 0.0, acc1 = 0.0, acc2 = 0.0, acc3 = 0.0;
      const float* tr = t_lds + lane * stride;
      const float* qr = q_lds + wave * 4 * GP_FEATURE_MAX_DIM;
      for (int j = 0; j < dim; j++) {
        const double tv = (double)tr[j];
        const double d0 = (double)qr[j] - tv, d1 = (double)qr[GP_FEATURE_MAX_DIM + j] - tv, d2 = (double)qr[2 * GP_FEATURE_MAX_DIM + j] - tv,
                     d3 = (double)qr[3 * GP_FEATURE_MAX_DIM + j] - tv;
        acc0 = fma(d0, d0, acc0);
        acc1 = fma(d1, d1, acc1);
        acc2 = fma(d2, d2, acc2);
        acc3 = fma(d3, d3, acc3);
      }
      const int ti = t0 + lane;
      if (acc0 < best[0]) best[0] = acc0, best_i[0] = ti;
      if (acc1 < best[1]) best[1] = acc1, best_i[1] = ti;
      if (acc2 < best[2]) best[2] = acc2, best_i[2] = ti;
      if (acc3 < best[3]) best[3] = acc3, best_i[3] = ti;
    }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) {
    double d = best[k];
    int bi = best_i[k];
    for (int off = 32; off > 0; off >>= 1) {
      const double od = __shfl_xor(d, off);
      const int oi = __shfl_xor(bi, off);
      if (oi >= 0 && (bi < 0 || od < d || (od == d && oi < bi))) d = od, bi = oi;
    }
    const int qi = q0 + wave * 4 + k;
    if (lane == 0 && qi < nq) {
      out_index[qi] = bi;
      out_sq_dist[qi] = bi >= 0 ? d : (double)INFINITY;
    }
  }
}

int launch_feature_nn(const float* target, int nt, const float* query, int num_rows, int dim, const int* rows, int nq, const int* stop, int* out_index, double* out_sq_dist,
                      hipStream_t stream) {
  hipLaunchKernelGGL(feature_nn_kernel, dim3(blocks_of(nq, kMatchQueries)), dim3(256), 0, stream, target, nt, query, num_rows, dim, rows, nq, stop, out_index, out_sq_dist);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // namespace gp

extern "C" int gp_feature_nn_search(const float* target_features_dev, int num_target, const float* query_features_dev, int num_query_rows, int dim, const int* rows_dev,
                                    int num_queries, int* indices_out_dev, double* sq_dists_out_dev, gp_stream_t stream) {
  if (dim < 1 || dim > GP_FEATURE_MAX_DIM) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: dim must be 1 .. 128");
  if (num_target < 1 || !target_features_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: no target features");
  if (num_queries < 0 || num_query_rows < 0 || (num_queries > 0 && (!query_features_dev || !indices_out_dev || !sq_dists_out_dev)))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: bad arguments");
  if (!rows_dev && num_queries > num_query_rows) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_feature_nn_search: more queries than query rows");
  if (num_queries == 0) return GP_OK;
  return gp::launch_feature_nn(target_features_dev, num_target, query_features_dev, num_query_rows, dim, rows_dev, num_queries, nullptr, indices_out_dev, sq_dists_out_dev,
                               (hipStream_t)stream);
}
