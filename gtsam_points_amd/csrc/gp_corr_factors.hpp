// gp_corr_factors.hpp -- what the single-factor entry points of the matching-cost factors (gp_corr_factors.hip, gp_colored_factors.hip, gp_ct_factors.hip) share with
// their batch (gp_corr_batch.hip): the per-point terms of GICP, ICP and LOAM, the reduction of a tile's sums into its partial row, the core every factor handle is
// built on (with the tail of a synchronous pass and the mapped result block) and the handles the batch borrows.
#pragma once
#include <cmath>
#include <cstring>
#include <memory>

#include "gp_corr_update.hpp"
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
  static constexpr int kNeighbours = 1;

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
  static constexpr int kNeighbours = 1;

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

// ---- the LOAM terms (integrated_loam_factor_impl.hpp) on the K = 2 / 3 nearest target points of a source point, stored int[K][n]: a term is handed corr + i and the
// stride n, slot 0 (>= 0, checked by the tile kernel) being the anchor x_j.  Both are the correspondence algebra above with another M, so they go through
// accumulate_sums in every mode: error = d^T M d, H = sum J^T M J, b = sum J^T M d with d = x_j - q, q = T p, J_t = [-[q]x, I], J_s = [R [p]x, -R].
// M is formed in f64 from the f32 target points.  Degenerate neighbours (x_j = x_l; a collinear triple) are not guarded, as in the reference: the division yields
// non-finite values that flow into the sums.
struct LoamDesc {
  const float* points;         // [n][3] source
  const float* target_points;  // [num_target][3]
};

// Point-to-edge (:300-365): v = x_j - x_l, c = 1 / |v|, r = c (q - x_j) x (q - x_l) = A d with A = c [v]x (J_e = [v]x, :350-353), so M = A^T A = c^2 [v]x^T [v]x
// = c^2 (|v|^2 I - v v^T), a full symmetric matrix.
struct LoamEdgeTerm {
  LoamDesc f;
  static constexpr int kErrRegs = 2;
  static constexpr int kNeighbours = 2;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, const int* __restrict__ c, size_t stride, const Pose& Tl, const Pose& Te, double* acc) const {
    const size_t j = (size_t)c[0], l = (size_t)c[stride];
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double jx = (double)f.target_points[3 * j], jy = (double)f.target_points[3 * j + 1], jz = (double)f.target_points[3 * j + 2];
    const double vx = jx - (double)f.target_points[3 * l], vy = jy - (double)f.target_points[3 * l + 1], vz = jz - (double)f.target_points[3 * l + 2];
    const double ci = 1.0 / sqrt(vx * vx + vy * vy + vz * vz);
    const double c2 = ci * ci;
    const double m[6] = {c2 * (vy * vy + vz * vz), -c2 * (vx * vy), -c2 * (vx * vz), c2 * (vx * vx + vz * vz), -c2 * (vy * vz), c2 * (vx * vx + vy * vy)};
    const double qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    const double qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    const double qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
    accumulate_sums<MODE>(Tl, m, px, py, pz, qx, qy, qz, jx - qx, jy - qy, jz - qz, acc);
  }
};

// Point-to-plane (:127-194): n = normalize((x_j - x_l) x (x_j - x_m)), r = n o (x_j - q) element-wise: the point-to-plane ICP term with the normal formed from
// the three neighbours instead of read from the cloud, M = diag(n o n).
struct LoamPlaneTerm {
  LoamDesc f;
  static constexpr int kErrRegs = 2;
  static constexpr int kNeighbours = 3;

  template <int MODE>
  __device__ __forceinline__ void accumulate(int i, const int* __restrict__ c, size_t stride, const Pose& Tl, const Pose& Te, double* acc) const {
    const size_t j = (size_t)c[0], l = (size_t)c[stride], mm = (size_t)c[2 * stride];
    const double px = (double)f.points[3 * (size_t)i], py = (double)f.points[3 * (size_t)i + 1], pz = (double)f.points[3 * (size_t)i + 2];
    const double jx = (double)f.target_points[3 * j], jy = (double)f.target_points[3 * j + 1], jz = (double)f.target_points[3 * j + 2];
    const double ax = jx - (double)f.target_points[3 * l], ay = jy - (double)f.target_points[3 * l + 1], az = jz - (double)f.target_points[3 * l + 2];
    const double bx = jx - (double)f.target_points[3 * mm], by = jy - (double)f.target_points[3 * mm + 1], bz = jz - (double)f.target_points[3 * mm + 2];
    double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
    const double norm = sqrt(nx * nx + ny * ny + nz * nz);
    nx /= norm, ny /= norm, nz /= norm;
    const double m[6] = {nx * nx, 0.0, 0.0, ny * ny, 0.0, nz * nz};
    const double qx = Te.r00 * px + Te.r01 * py + Te.r02 * pz + Te.tx;
    const double qy = Te.r10 * px + Te.r11 * py + Te.r12 * pz + Te.ty;
    const double qz = Te.r20 * px + Te.r21 * py + Te.r22 * pz + Te.tz;
    accumulate_sums<MODE>(Tl, m, px, py, pz, qx, qy, qz, jx - qx, jy - qy, jz - qz, acc);
  }
};

// IntegratedLOAMFactor_::validate_correspondences (:487-529) on the stored correspondences of one source point (c = corr + i, int[K][n]): with
// theta(p) = atan2(p.z, hypot(p.x, p.y)) in f64, an edge pair is rejected (every slot -1) when |theta_j - theta_l| < 0.1 pi / 180, a plane triple when that holds
// and |theta_j - theta_m| < 0.1 * pi * 180.  The second bound is the reference's expression AS WRITTEN (about 56.5 rad: it always holds); parity is the target.
// Idempotent: a rejected point is skipped.
__device__ __forceinline__ void loam_validate_point(const float* __restrict__ target_points, int* __restrict__ c, size_t stride, int K) {
  const int j = c[0];
  if (j < 0) return;
  auto theta = [&](int t) {
    const double x = (double)target_points[3 * (size_t)t], y = (double)target_points[3 * (size_t)t + 1], z = (double)target_points[3 * (size_t)t + 2];
    return atan2(z, hypot(x, y));
  };
  const double tj = theta(j);
  bool reject = fabs(tj - theta(c[stride])) < 0.1 * M_PI / 180.0;
  if (K == 3) reject = reject && fabs(tj - theta(c[2 * stride])) < 0.1 * M_PI * 180.0;
  if (reject)
    for (int k = 0; k < K; k++) c[(size_t)k * stride] = -1;
}

// the lanes meet in the butterfly / shuffle tree and the four waves in wave order: a fixed order, two passes over the same correspondences are bit-identical
// (row: where the workgroup's sums go -- the single-factor kernels' row is their blockIdx.x, a batch's tile carries its own)
template <int MODE>
__device__ __forceinline__ void store_tile_sums_row(double* acc, double* __restrict__ row) {
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
      const double v = wave_sum(acc[k]);
      if (lane == 0) lds[wave][k] = v;
    }
  }
  __syncthreads();
  if (threadIdx.x < STRIDE) {
    double s = 0.0;
    if (threadIdx.x < NACC) s = (lds[0][threadIdx.x] + lds[1][threadIdx.x]) + (lds[2][threadIdx.x] + lds[3][threadIdx.x]);
    row[threadIdx.x] = s;
  }
}
template <int MODE>
__device__ __forceinline__ void store_tile_sums(double* acc, double* __restrict__ partials) {
  constexpr int STRIDE = MODE == MODE_LIN_GENERAL ? ACCG_STRIDE : ACC_STRIDE;
  store_tile_sums_row<MODE>(acc, partials + (size_t)blockIdx.x * STRIDE);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side: the factor handles
// ---------------------------------------------------------------------------------------------------------------

namespace gp {

// where a synchronous call's kernels leave its result: a block and its completion words (gp_vgicp_shared.hpp: DoneFlags) in host-mapped pinned memory, with the
// device's pointers to both and the call's sequence number.  The single factors keep one record and one word, their batch one of each per member.
struct MappedResults {
  PinnedArray out, done;
  void *out_dev = nullptr, *done_dev = nullptr;
  unsigned long long seq = 0;
  int ensure(size_t out_bytes, size_t words) {
    GP_TRY(out.ensure(out_bytes));
    GP_HIP(hipHostGetDevicePointer(&out_dev, out.ptr, 0));
    GP_TRY(done.ensure(sizeof(unsigned long long) * words));
    memset(done.ptr, 0, done.bytes);
    GP_HIP(hipHostGetDevicePointer(&done_dev, done.ptr, 0));
    return GP_OK;
  }
  DoneFlags next() { return DoneFlags{static_cast<unsigned long long*>(done_dev), ++seq}; }
  const unsigned long long* words() const { return static_cast<const unsigned long long*>(done.ptr); }
};

}  // namespace gp

// what every factor keeps: the search's inputs, the stored correspondences and the pose they belong to, the tile geometry and where a pass leaves its result
struct gp_corr_factor_core {
  const gp_point_grid* grid = nullptr;  // the search structure over the target (the cut-off ends every search, whatever cell size it was built with)
  const float* points = nullptr;        // [n][3] source
  int n = 0;
  double max_sq_dist = 0.0;
  hipStream_t stream = nullptr;
  int tile_points = 1024;
  int num_tiles = 0;
  gp::DeviceArray partials, corr;  // corr: [n] correspondences of the last correspondence pass
  gp::MappedResults res;           // one record (or one error) and the completion word of the synchronous calls
  gp_corr_update upd;              // (a LOAM part leaves its own unused: gp_loam_factor keeps one for both parts)
  int num_inliers = 0;             // of the last linearise
  // the photometric factors handed an XYZI structure (gp_intensity_search.hip; BORROWED): search() runs the 4-D walk with the source's intensities, `grid` is unused
  const gp_intensity_grid* xyzi = nullptr;
  const float* intensities = nullptr;  // [n] source

  int prepare(const gp_point_grid* grid_, const float* points_dev, int n_, double max_sq_dist_, hipStream_t stream_) {
    grid = grid_;
    points = points_dev;
    n = n_;
    max_sq_dist = max_sq_dist_;
    stream = stream_;
    num_tiles = (n + tile_points - 1) / tile_points;
    GP_TRY(partials.alloc(sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(num_tiles, 1)));
    GP_TRY(corr.alloc(sizeof(int) * (size_t)std::max(n, 1)));
    return res.ensure(sizeof(gp_linearized6), 1);
  }

  // the correspondence pass at pose_lin (n > 0): the one place that picks the launch
  int search(const double* pose_lin) {
    if (xyzi)
      GP_TRY(gp::launch_nearest_correspondences_xyzi(xyzi, points, intensities, n, pose_lin, max_sq_dist, corr.as<int>(), stream));
    else
      GP_TRY(gp::launch_nearest_correspondences(grid, points, n, pose_lin, max_sq_dist, corr.as<int>(), stream));
    upd.note_search(pose_lin);
    return GP_OK;
  }

  // the correspondence pass of the LOAM parts at pose_lin (n > 0): the k nearest into corr (int[k][n], allocated by the part); the pose is kept by the factor
  int search_k(int k, const double* pose_lin) { return gp::launch_nearest_k_correspondences(grid, points, n, k, pose_lin, max_sq_dist, corr.as<int>(), stream); }

  // One synchronous pass over the stored correspondences (gp_corr_tile.hpp: defined there for the units that instantiate it with their terms).
  template <class TERM>
  int run_pass(const TERM& term, const double* pose_lin, const double* pose_eval, void* out_host);

  // The tail of a synchronous pass, behind the tile kernel: the partial rows finalised into the mapped block -- the error (out_host a double), or the record at
  // pose_lin (a gp_linearized6; general: the rows hold the 92 explicit sums, whose expansion does not read the pose) --, the wait for the completion word, the copy out.
  int finish_pass(bool error, const double* pose_lin, bool general, void* out_host) {
    const gp::DoneFlags done = res.next();
    if (error)
      GP_TRY(gp::launch_finalize_error_single(stream, partials.as<double>(), num_tiles, reinterpret_cast<double*>(res.out_dev), done));
    else
      GP_TRY(gp::launch_finalize_single(stream, nullptr, pose_lin, partials.as<double>(), num_tiles, reinterpret_cast<gp_linearized6*>(res.out_dev), general, done));
    GP_TRY(gp::wait_done(res.words(), 1, done.seq, stream, 100 + (long)num_tiles * (long)tile_points / 1000));  // spin budget ~4x the kernel (0.2 ns per point)
    memcpy(out_host, res.out.ptr, error ? sizeof(double) : sizeof(gp_linearized6));
    return GP_OK;
  }
};

// what every gp_*_destroy of this family does: the handle's stream runs dry, then the handle goes (a borrowed grid or member stays the caller's)
template <class HANDLE>
int gp_corr_destroy(HANDLE* h) {
  if (!h) return GP_OK;
  (void)hipStreamSynchronize(h->stream);
  delete h;
  return GP_OK;
}

// set_correspondence_update_tolerance of the factor `who` (u: its update rule, null for a null handle)
inline int gp_corr_set_update_tolerance(gp_corr_update* u, double angle, double trans, const char* who) {
  if (!u) return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string(who) + ": null");
  u->tol_rot = angle;
  u->tol_trans = trans;
  return GP_OK;
}

// The single factors on ONE nearest neighbour: the core, the per-point term and the pass that picks its tile kernel (each defined in the unit that instantiates the
// kernels).  gp_corr_tile.hpp's corr_factor_linearize / _compute_error drive all three.
struct gp_gicp_factor : gp_corr_factor_core {  // (zero update tolerances, never set: every linearise searches)
  gp_point_grid* own_grid = nullptr;            // OWNED: the factor's target 1-NN structure
  gp::GicpTerm term{};
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host);  // (gp_corr_factors.hip)
  ~gp_gicp_factor() {
    if (own_grid) gp_point_grid_destroy(own_grid);
  }
};

struct gp_icp_factor : gp_corr_factor_core {  // (the grid is BORROWED: the reference's target_tree, shared between factors)
  gp::IcpDesc desc{};
  bool plane = false;
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host);  // (gp_corr_factors.hip)
};

// IntegratedPointToEdgeFactor_ (k = 2) / IntegratedPointToPlaneFactor_ (k = 3) as one part of a gp_loam_factor: the core with corr as int[k][n]
struct gp_loam_part : gp_corr_factor_core {
  int k = 0;
  gp::LoamDesc desc{};
  int run_pass(const double* pose_lin, const double* pose_eval, void* out_host);  // (gp_corr_factors.hip)
  int validate();                                                                 // (gp_corr_factors.hip) the validation kernel over corr, asynchronous
};

// IntegratedLOAMFactor_: an edge part and a plane part (either may be absent: the two single factors), both grids BORROWED.  What the two parts decide together --
// the pose of the stored correspondences, the update tolerances, the validation -- is kept here.
struct gp_loam_factor {
  std::unique_ptr<gp_loam_part> edge, plane;
  hipStream_t stream = nullptr;
  bool validation = false;  // enable_correspondence_validation (off by default, :385)
  gp_corr_update upd;
  int num_edges = 0, num_planes = 0;  // inliers of the last linearise, per part
};
