// gp_feature_match.hpp -- the launch of the exact feature search (gp_feature_match.hip) for the units that match on their own stream: RANSAC (gp_registration.hip) and
// the correspondences of gp_gnc.hip.
#pragma once

#include "gp_host.hpp"

namespace gp {

// one launch of feature_nn_kernel (the contract of gp_feature_nn_search; stop: a device flag read first, or NULL).  Asynchronous on `stream`.
int launch_feature_nn(const float* target, int nt, const float* query, int num_rows, int dim, const int* rows, int nq, const int* stop, int* out_index, double* out_sq_dist,
                      hipStream_t stream);

}  // namespace gp
