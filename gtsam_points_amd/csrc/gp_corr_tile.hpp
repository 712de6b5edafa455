// gp_corr_tile.hpp -- the tile kernel over stored correspondences, the synchronous pass that launches it and the single factors' update rule around that pass, for
// the translation units that instantiate them with their terms: gp_corr_factors.hip (GICP, ICP, LOAM) and gp_colored_factors.hip (colored GICP).  A unit's kernel-resource remarks list its own instantiations only.
#pragma once
#include "gp_corr_factors.hpp"

namespace gp {

// One workgroup per tile of `tile_points` points, lane t of 256 takes points t, t + 256, ... of its tile and skips those without a target point within the cut-off
// (integrated_gicp_factor_impl.hpp:166-170, integrated_icp_factor_impl.hpp:200-202).
template <int MODE, class TERM>  // MODE_LIN (rigid pose: 29 sums + adjoint finalize), MODE_ERR, MODE_LIN_GENERAL (any 3x3 block: 92 explicit sums)
__global__ void __launch_bounds__(256) corr_tile_kernel(TERM f, const CorrPoses poses, int n, int tile_points, double* __restrict__ partials, const int* __restrict__ corr) {
  constexpr int NREG = MODE == MODE_LIN_GENERAL ? ACCG_SIZE : (MODE == MODE_ERR ? TERM::kErrRegs : 32);
  const Pose Tl = load_pose(poses.lin);
  const Pose Te = MODE == MODE_ERR ? load_pose(poses.eval) : Tl;
  double acc[NREG];
#pragma unroll
  for (int k = 0; k < NREG; k++) acc[k] = 0.0;
  const int begin = blockIdx.x * tile_points;
  const int end = min(begin + tile_points, n);
  for (int i = begin + threadIdx.x; i < end; i += 256) {
    const int c = corr[i];
    if (c < 0) continue;
    if constexpr (TERM::kNeighbours == 1)
      f.template accumulate<MODE>(i, (size_t)c, Tl, Te, acc);
    else  // (the LOAM terms: corr is int[K][n], slot 0 the anchor)
      f.template accumulate<MODE>(i, corr + i, (size_t)n, Tl, Te, acc);
  }
  store_tile_sums<MODE>(acc, partials);
}

}  // namespace gp

// One synchronous pass over the stored correspondences.  pose_eval == nullptr: a linearise at pose_lin, out_host is a gp_linearized6; otherwise the error at
// pose_eval, out_host is a double.  The 29-sum kernel + adjoint finalize is exact only for an orthonormal 3x3 block; any other pose (e.g. built from 6-digit
// quaternions, src/test/test_matching_cost_factors.cpp:50-55) takes the 92-sum path with the explicit J_s, like the VGICP factor.
template <class TERM>
int gp_corr_factor_core::run_pass(const TERM& term, const double* pose_lin, const double* pose_eval, void* out_host) {
  gp::CorrPoses P;
  memcpy(P.lin, pose_lin, sizeof(double) * 16);
  memcpy(P.eval, pose_eval ? pose_eval : pose_lin, sizeof(double) * 16);
  const bool rigid = gp::pose_is_rigid(pose_lin);
  if (num_tiles > 0) {
    if (pose_eval)
      hipLaunchKernelGGL((gp::corr_tile_kernel<gp::MODE_ERR, TERM>), dim3(num_tiles), dim3(256), 0, stream, term, P, n, tile_points, partials.as<double>(), corr.as<int>());
    else if (rigid)
      hipLaunchKernelGGL((gp::corr_tile_kernel<gp::MODE_LIN, TERM>), dim3(num_tiles), dim3(256), 0, stream, term, P, n, tile_points, partials.as<double>(), corr.as<int>());
    else
      hipLaunchKernelGGL((gp::corr_tile_kernel<gp::MODE_LIN_GENERAL, TERM>), dim3(num_tiles), dim3(256), 0, stream, term, P, n, tile_points, partials.as<double>(), corr.as<int>());
    GP_HIP(hipGetLastError());
  }
  return finish_pass(pose_eval != nullptr, pose_lin, !rigid, out_host);
}

// The update rule of the single factors on one nearest neighbour (GICP, ICP, colored GICP; F: the handle), gp_corr_update deciding.  A linearise searches unless the
// update tolerances keep the stored correspondences (GICP's are zero: it always searches -- IntegratedGICPFactor_::linearize calls update_correspondences every
// time); an error evaluation re-uses the stored correspondences when they belong to its linearisation pose -- the reference's error() evaluates on those of the
// last linearise (integrated_gicp_factor_impl.hpp:183-185) -- and searches at pose_lin otherwise.
template <class F>
int corr_factor_linearize(F* f, const double* pose, gp_linearized6* out_host) {
  if (f->num_tiles > 0 && !f->upd.keep(pose)) GP_TRY(f->search(pose));
  f->upd.note_linearize(pose);
  GP_TRY(f->run_pass(pose, nullptr, out_host));
  f->num_inliers = (int)out_host->num_inliers;
  return GP_OK;
}

template <class F>
int corr_factor_compute_error(F* f, const double* pose_lin, const double* pose_eval, double* out_host) {
  if (f->num_tiles > 0 && !f->upd.stored(pose_lin)) GP_TRY(f->search(pose_lin));
  return f->run_pass(pose_lin, pose_eval, out_host);
}
