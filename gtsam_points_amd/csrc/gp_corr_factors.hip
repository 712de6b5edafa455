// gp_corr_factors.hip -- the matching-cost factors on 1-NN correspondences: GICP and ICP (point-to-point and point-to-plane).
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/impl/integrated_gicp_factor_impl.hpp:132-296              GICP correspondences+H/b  -> gp_gicp_factor_*
//   factors/impl/integrated_icp_factor_impl.hpp:128-157,180-248       ICP correspondences+H/b   -> gp_icp_factor_*
//
// Nothing of the search lives here: gp::launch_nearest_correspondences (gp_knn.hip) writes, for the source points transformed by the linearisation pose, the index
// of the nearest target point within the cut-off into corr[]; a tile kernel then sums the factor's terms over those correspondences into the partial-row layout of
// the VGICP factor (gp_device.hpp ACC / ACCG), which goes through the same finalize kernels (gp_vgicp_shared.hpp).  The correspondence pass is its own kernel: with
// the search inlined the tile kernel held 157 VGPRs, and measured 0.233 against 0.160 ms per linearise (profiles/r02_gicp_split_ab.jsonl).  The stored
// correspondences are also what the reference's error() evaluates on (it does not search again).
#include <cmath>
#include <cstring>
#include <memory>

#include "gp_host.hpp"
#include "gp_vgicp_tile.hpp"

namespace gp {

// the poses ride in the kernel arguments (no H2D copy in front of the launch)
struct CorrPoses {
  double lin[16], eval[16];
};

// ---- the per-point terms: a descriptor of device arrays + "given source point i, its target point j, Tl and Te, accumulate into acc" ----

// GICP: the same H/b algebra as VGICP (integrated_gicp_factor_impl.hpp:199-296)
struct GicpTerm {
  const float* points;
  const float* covs;
  const float* target_points;
  const float* target_covs;
  static constexpr int kErrRegs = 32;  // accumulate_terms_mu<MODE_ERR> is handed the 32-register array of the linearise

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const Pose& Tl, const Pose& Te, double* acc) const {
    const GicpTerm& f = *this;
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double lx = Tl.r00 * px + Tl.r01 * py + Tl.r02 * pz + Tl.tx;
    const double ly = Tl.r10 * px + Tl.r11 * py + Tl.r12 * pz + Tl.ty;
    const double lz = Tl.r20 * px + Tl.r21 * py + Tl.r22 * pz + Tl.tz;
    const float* cp = f.covs + 9 * (size_t)i;
    const float* cq = f.target_covs + 9 * j;
    // reuse the VGICP per-point algebra: the "voxel" is the matched target point (mu_B, C_B)
    const double mux = (double)f.target_points[3 * j], muy = (double)f.target_points[3 * j + 1], muz = (double)f.target_points[3 * j + 2];
    // symmetric parts of both column-major 3x3 covariances (exactly the inputs when they are symmetric)
    const double cb[6] = {(double)cq[0], 0.5 * ((double)cq[3] + (double)cq[1]), 0.5 * ((double)cq[6] + (double)cq[2]),
                          (double)cq[4], 0.5 * ((double)cq[7] + (double)cq[5]), (double)cq[8]};
    if constexpr (MODE == MODE_LIN_GENERAL) {
      const double ca[6] = {(double)cp[0], 0.5 * ((double)cp[3] + (double)cp[1]), 0.5 * ((double)cp[6] + (double)cp[2]),
                            (double)cp[4], 0.5 * ((double)cp[7] + (double)cp[5]), (double)cp[8]};
      double m[6];
      fused_mahalanobis(Tl, ca, cb, m);
      accumulate_sums<MODE_LIN_GENERAL>(Tl, m, px, py, pz, lx, ly, lz, mux - lx, muy - ly, muz - lz, acc);
    } else {
      const v2d c01 = {cb[0], cb[1]}, c23 = {cb[2], cb[3]}, c45 = {cb[4], cb[5]};
      accumulate_terms_mu<MODE, double>(Tl, Te, (float)px, (float)py, (float)pz, cp, mux, muy, muz, c01, c23, c45, acc);
    }
  }
};

// The per-point body of IntegratedICPFactor_::evaluate (integrated_icp_factor_impl.hpp:199-240):
//   q = T p, d = mu_B - q, r = n_B o d (element-wise, :212; point-to-point: r = d), error += r^T r (:215, no 1/2),
//   J_t = diag(n_B) [-[q]x, I], J_s = diag(n_B) [R [p]x, -R] (:220-232), H += J^T J, b += J^T r (:234-238).
// That is the GICP algebra with M = diag(n_B o n_B) (or I) in place of the fused Mahalanobis matrix, so the sums go into the SAME
// partial-row layout and through the same finalize kernels: b_t = [q x w; w] with w = n_B o r = M d,
// K = M [q]x and TL = -[q]x K written out for a diagonal M (the off-diagonal slots of ACC_M and the diagonal of K stay zero).
// A matched point costs 4 B (index) + 12 B (source point) + 12 B (target point) [+ 12 B (normal)]; no covariance is read and nothing is
// inverted.  A non-orthonormal 3x3 block takes the 92 explicit sums of accumulate_sums<MODE_LIN_GENERAL>, J_s from the block AS GIVEN.
struct IcpDesc {
  const float* points;          // [n][3] source
  const float* target_points;   // [num_target][3]
  const float* target_normals;  // [num_target][3]; read by the point-to-plane kernels only
};
template <bool PLANE>
struct IcpTerm {
  IcpDesc f;
  static constexpr int kErrRegs = 2;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, size_t j, const Pose& Tl, const Pose& Te, double* acc) const {
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double mux = (double)f.target_points[3 * j], muy = (double)f.target_points[3 * j + 1], muz = (double)f.target_points[3 * j + 2];
    double nx = 1.0, ny = 1.0, nz = 1.0;
    if constexpr (PLANE) {
      nx = (double)f.target_normals[3 * j];
      ny = (double)f.target_normals[3 * j + 1];
      nz = (double)f.target_normals[3 * j + 2];
    }
    const double qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    const double qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    const double qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
    const double dx = mux - qx, dy = muy - qy, dz = muz - qz;
    if constexpr (MODE == MODE_LIN_GENERAL) {
      const double m[6] = {nx * nx, 0.0, 0.0, ny * ny, 0.0, nz * nz};
      accumulate_sums<MODE_LIN_GENERAL>(Tl, m, px, py, pz, qx, qy, qz, dx, dy, dz, acc);
    } else {
      const double rx = PLANE ? nx * dx : dx, ry = PLANE ? ny * dy : dy, rz = PLANE ? nz * dz : dz;  // r = n_B o d
      acc[ACC_COUNT] += 1.0;
      acc[ACC_ERR] += rx * rx + ry * ry + rz * rz;
      if constexpr (MODE == MODE_LIN) {
        const double m0 = PLANE ? nx * nx : 1.0, m3 = PLANE ? ny * ny : 1.0, m5 = PLANE ? nz * nz : 1.0;  // M = diag(n_B o n_B)
        const double wx = PLANE ? nx * rx : rx, wy = PLANE ? ny * ry : ry, wz = PLANE ? nz * rz : rz;     // w = n_B o r
        acc[ACC_M + 0] += m0;
        acc[ACC_M + 3] += m3;
        acc[ACC_M + 5] += m5;
        // K = M [q]x, row-major
        const double k01 = -m0 * qz, k02 = m0 * qy, k10 = m3 * qz, k12 = -m3 * qx, k20 = -m5 * qy, k21 = m5 * qx;
        acc[ACC_K + 1] += k01;
        acc[ACC_K + 2] += k02;
        acc[ACC_K + 3] += k10;
        acc[ACC_K + 5] += k12;
        acc[ACC_K + 6] += k20;
        acc[ACC_K + 7] += k21;
        // TL = -[q]x K (= [q]x^T M [q]x), upper triangle
        acc[ACC_TL + 0] += qz * k10 - qy * k20;
        acc[ACC_TL + 1] += -qy * k21;
        acc[ACC_TL + 2] += qz * k12;
        acc[ACC_TL + 3] += qx * k21 - qz * k01;
        acc[ACC_TL + 4] += -qz * k02;
        acc[ACC_TL + 5] += qy * k02 - qx * k12;
        // b_t = [q x w; w]
        acc[ACC_QXMR + 0] += qy * wz - qz * wy;
        acc[ACC_QXMR + 1] += qz * wx - qx * wz;
        acc[ACC_QXMR + 2] += qx * wy - qy * wx;
        acc[ACC_MR + 0] += wx;
        acc[ACC_MR + 1] += wy;
        acc[ACC_MR + 2] += wz;
      }
    }
  }
};

// the lanes meet in the butterfly / shuffle tree and the four waves in wave order: a fixed order, two passes over the same correspondences are bit-identical
template <int MODE>
__device__ __forceinline__ void store_tile_sums(double* acc, double* __restrict__ partials) {
  constexpr int NACC = MODE == MODE_ERR ? 2 : (MODE == MODE_LIN ? ACC_SIZE : ACCG_SIZE);
  constexpr int STRIDE = MODE == MODE_LIN_GENERAL ? ACCG_STRIDE : ACC_STRIDE;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  __shared__ double lds[4][STRIDE];
  if constexpr (MODE == MODE_LIN) {
    const double s = butterfly_reduce32(acc, lane);
    if ((lane & 1) == 0) lds[wave][butterfly_component(lane)] = s;
  } else {
#pragma unroll
    for (int k = 0; k < NACC; k++) {
      double v = acc[k];
#pragma unroll
      for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
      if (lane == 0) lds[wave][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < STRIDE) {
    double s = 0.0;
    if (threadIdx.x < NACC) s = (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
    partials[(size_t)blockIdx.x * STRIDE + threadIdx.x] = s;
  }
}

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
    f.template accumulate<MODE>(i, (size_t)c, Tl, Te, acc);
  }
  store_tile_sums<MODE>(acc, partials);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

// what both factors keep: the search's inputs, the stored correspondences and the pose they belong to, the tile geometry and where a pass leaves its result
struct gp_corr_factor_core {
  const gp_point_grid* grid = nullptr;  // the search structure over the target (the cut-off ends every search, whatever cell size it was built with)
  const float* points = nullptr;        // [n][3] source
  int n = 0;
  double max_sq_dist = 0.0;
  hipStream_t stream = nullptr;
  int tile_points = 1024;
  int num_tiles = 0;
  gp::DeviceArray partials, corr;  // corr: [n] correspondences of the last correspondence pass
  gp::PinnedArray h_out;
  void* h_out_dev = nullptr;
  gp::PinnedArray h_done;  // completion word of the synchronous calls (gp_vgicp_shared.hpp: DoneFlags)
  void* h_done_dev = nullptr;
  unsigned long long seq = 0;
  double corr_pose[16] = {0};  // last_correspondence_point: the pose the stored correspondences were searched at
  bool corr_valid = false;

  int prepare(const gp_point_grid* grid_, const float* points_dev, int n_, double max_sq_dist_, hipStream_t stream_) {
    grid = grid_;
    points = points_dev;
    n = n_;
    max_sq_dist = max_sq_dist_;
    stream = stream_;
    num_tiles = (n + tile_points - 1) / tile_points;
    GP_TRY(partials.alloc(sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(num_tiles, 1)));
    GP_TRY(corr.alloc(sizeof(int) * (size_t)std::max(n, 1)));
    GP_TRY(h_out.ensure(sizeof(gp_linearized6)));
    GP_HIP(hipHostGetDevicePointer(&h_out_dev, h_out.ptr, 0));
    GP_TRY(h_done.ensure(sizeof(unsigned long long)));
    memset(h_done.ptr, 0, h_done.bytes);
    GP_HIP(hipHostGetDevicePointer(&h_done_dev, h_done.ptr, 0));
    return GP_OK;
  }

  bool searched_at(const double* pose) const { return corr_valid && memcmp(corr_pose, pose, sizeof(double) * 16) == 0; }

  // the correspondence pass at pose_lin (n > 0)
  int search(const double* pose_lin) {
    GP_TRY(gp::launch_nearest_correspondences(grid, points, n, pose_lin, max_sq_dist, corr.as<int>(), stream));
    memcpy(corr_pose, pose_lin, sizeof(double) * 16);
    corr_valid = true;
    return GP_OK;
  }

  // One synchronous pass over the stored correspondences.  pose_eval == nullptr: a linearise at pose_lin, out_host is a gp_linearized6; otherwise the error at
  // pose_eval, out_host is a double.  The 29-sum kernel + adjoint finalize is exact only for an orthonormal 3x3 block; any other pose (e.g. built from 6-digit
  // quaternions, src/test/test_matching_cost_factors.cpp:50-55) takes the 92-sum path with the explicit J_s, like the VGICP factor.
  template <class TERM>
  int run_pass(const TERM& term, const double* pose_lin, const double* pose_eval, void* out_host) {
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
    const gp::DoneFlags done{static_cast<unsigned long long*>(h_done_dev), ++seq};
    if (pose_eval)
      GP_TRY(gp::launch_finalize_error_single(stream, partials.as<double>(), num_tiles, reinterpret_cast<double*>(h_out_dev), done));
    else
      GP_TRY(gp::launch_finalize_single(stream, nullptr, pose_lin, partials.as<double>(), num_tiles, reinterpret_cast<gp_linearized6*>(h_out_dev), !rigid, done));
    GP_TRY(gp::wait_done(static_cast<const unsigned long long*>(h_done.ptr), 1, done.seq, stream, 100 + (long)num_tiles * (long)tile_points / 1000));  // spin budget ~4x the kernel (0.2 ns per point)
    memcpy(out_host, h_out.ptr, pose_eval ? sizeof(double) : sizeof(gp_linearized6));
    return GP_OK;
  }
};

struct gp_gicp_factor : gp_corr_factor_core {
  gp_point_grid* own_grid = nullptr;  // OWNED: the factor's target 1-NN structure
  gp::GicpTerm term{};
  ~gp_gicp_factor() {
    if (own_grid) gp_point_grid_destroy(own_grid);
  }
};

struct gp_icp_factor : gp_corr_factor_core {  // (the grid is BORROWED: the reference's target_tree, shared between factors)
  gp::IcpDesc desc{};
  bool plane = false;
  double lin_pose[16] = {0};  // the pose of the last linearise (which may have kept older correspondences: the update tolerances)
  bool lin_valid = false;
  double tol_rot = 0.0, tol_trans = 0.0;  // correspondence_update_tolerance_rot / _trans (:32-33)
  int num_correspondences = 0;
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host) {
    if (plane) return gp_corr_factor_core::run_pass(gp::IcpTerm<true>{desc}, pose_lin, pose_eval, out_host);
    return gp_corr_factor_core::run_pass(gp::IcpTerm<false>{desc}, pose_lin, pose_eval, out_host);
  }
};

// update_correspondences' decision (integrated_icp_factor_impl.hpp:129-137) on two column-major 4x4 poses: diff = delta^-1 * last (the
// isometry inverse, R^T and -R^T t), its rotation angle and the norm of its translation against the tolerances, both strict
static bool icp_keep_correspondences(const gp_icp_factor* f, const double* delta) {
  if (!f->corr_valid || !(f->tol_trans > 0.0 || f->tol_rot > 0.0)) return false;
  const double* last = f->corr_pose;
  double D[3][3], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) D[r][c] = delta[4 * r] * last[4 * c] + delta[4 * r + 1] * last[4 * c + 1] + delta[4 * r + 2] * last[4 * c + 2];
    t[r] = delta[4 * r] * (last[12] - delta[12]) + delta[4 * r + 1] * (last[13] - delta[13]) + delta[4 * r + 2] * (last[14] - delta[14]);
  }
  // angle in [0, pi] from sin (the skew part) and cos (the trace): what Eigen::AngleAxisd(diff.linear()).angle() gives for a rotation
  const double sx = 0.5 * (D[2][1] - D[1][2]), sy = 0.5 * (D[0][2] - D[2][0]), sz = 0.5 * (D[1][0] - D[0][1]);
  const double diff_rot = std::atan2(std::sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (D[0][0] + D[1][1] + D[2][2] - 1.0));
  const double diff_trans = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
  return diff_rot < f->tol_rot && diff_trans < f->tol_trans;
}

extern "C" {

// ---- GICP factor ----------------------------------------------------------------------------------------------------

int gp_gicp_factor_create(const float* target_points_dev, const float* target_covs_dev, int n_target, const float* points_dev, const float* covs_dev, int n,
                          double max_correspondence_distance_sq, gp_stream_t stream, gp_gicp_factor_t** out) {
  return gp_gicp_factor_create_ex(target_points_dev, target_covs_dev, n_target, points_dev, covs_dev, n, max_correspondence_distance_sq, 0, nullptr, stream, out);
}

int gp_gicp_factor_create_ex(const float* target_points_dev, const float* target_covs_dev, int n_target, const float* points_dev, const float* covs_dev, int n,
                             double max_correspondence_distance_sq, int structure, unsigned long long* counters_dev, gp_stream_t stream, gp_gicp_factor_t** out) {
  if (!target_points_dev || !target_covs_dev || !points_dev || !covs_dev || n < 0 || n_target < 0 || !(max_correspondence_distance_sq > 0.0) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_gicp_factor_create: bad arguments");
  auto f = std::make_unique<gp_gicp_factor>();
  // cell = 1/4 of the correspondence radius: the fine shells 0 and 1 settle the well-matched points, and one block edge = the
  // radius, so the block walk behind them ends at the first block shell at the latest
  GP_TRY(gp_point_grid_create_ex(target_points_dev, n_target, std::sqrt(max_correspondence_distance_sq) / 4.0, structure, counters_dev, stream, &f->own_grid));
  f->term = {points_dev, covs_dev, target_points_dev, target_covs_dev};
  GP_TRY(f->prepare(f->own_grid, points_dev, n, max_correspondence_distance_sq, (hipStream_t)stream));
  *out = f.release();
  return GP_OK;
}

int gp_gicp_factor_destroy(gp_gicp_factor_t* f) {
  if (!f) return GP_OK;
  (void)hipStreamSynchronize(f->stream);
  delete f;  // (and its grid)
  return GP_OK;
}

// A linearise always searches (IntegratedGICPFactor_::linearize calls update_correspondences every time, the default update tolerances being zero); an error
// evaluation re-uses the stored correspondences when they belong to its linearisation pose -- the reference's error() evaluates on the correspondences of the
// last linearise (impl.hpp:183-185).
int gp_gicp_factor_linearize(gp_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_gicp_factor_linearize: null");
  if (f->num_tiles > 0) GP_TRY(f->search(pose));
  return f->run_pass(f->term, pose, nullptr, out_host);
}

int gp_gicp_factor_compute_error(gp_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_gicp_factor_compute_error: null");
  if (f->num_tiles > 0 && !f->searched_at(pose_lin)) GP_TRY(f->search(pose_lin));
  return f->run_pass(f->term, pose_lin, pose_eval, out_host);
}

// ---- ICP factor -----------------------------------------------------------------------------------------------------

int gp_icp_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, int n_target, const float* points_dev, int n,
                         double max_correspondence_distance_sq, int point_to_plane, gp_stream_t stream, gp_icp_factor_t** out) {
  if (!grid || !target_points_dev || !points_dev || n < 0 || n_target < 0 || !(max_correspondence_distance_sq > 0.0) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_create: bad arguments");
  if (point_to_plane && !target_normals_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_create: a point-to-plane factor needs the target's normals");
  auto f = std::make_unique<gp_icp_factor>();
  f->plane = point_to_plane != 0;
  f->desc = {points_dev, target_points_dev, target_normals_dev};
  GP_TRY(f->prepare(grid, points_dev, n, max_correspondence_distance_sq, (hipStream_t)stream));
  *out = f.release();
  return GP_OK;
}

int gp_icp_factor_destroy(gp_icp_factor_t* f) {
  if (!f) return GP_OK;
  (void)hipStreamSynchronize(f->stream);
  delete f;  // (the grid is the caller's)
  return GP_OK;
}

int gp_icp_factor_set_correspondence_update_tolerance(gp_icp_factor_t* f, double angle, double trans) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_set_correspondence_update_tolerance: null");
  f->tol_rot = angle;
  f->tol_trans = trans;
  return GP_OK;
}

int gp_icp_factor_num_correspondences(const gp_icp_factor_t* f) { return f ? f->num_correspondences : 0; }

int gp_icp_factor_linearize(gp_icp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_linearize: null");
  if (f->num_tiles > 0 && !icp_keep_correspondences(f, pose)) GP_TRY(f->search(pose));
  memcpy(f->lin_pose, pose, sizeof(double) * 16);
  f->lin_valid = true;
  GP_TRY(f->run_pass(pose, nullptr, out_host));
  f->num_correspondences = (int)out_host->num_inliers;
  return GP_OK;
}

int gp_icp_factor_compute_error(gp_icp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_compute_error: null");
  // the stored correspondences serve when pose_lin is the pose of the last linearise (which may itself have kept older ones) or the pose they were searched at
  const bool stored = f->corr_valid && ((f->lin_valid && memcmp(f->lin_pose, pose_lin, sizeof(double) * 16) == 0) || f->searched_at(pose_lin));
  if (f->num_tiles > 0 && !stored) {
    GP_TRY(f->search(pose_lin));
    f->lin_valid = false;
  }
  return f->run_pass(pose_lin, pose_eval, out_host);
}

}  // extern "C"
