// gp_corr_factors.hip -- the matching-cost factors on nearest-neighbour correspondences: GICP and ICP (point-to-point and point-to-plane) on the nearest target point,
// the LOAM point-to-edge and point-to-plane factors on the 2 and 3 nearest.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/impl/integrated_gicp_factor_impl.hpp:132-296              GICP correspondences+H/b  -> gp_gicp_factor_*
//   factors/impl/integrated_icp_factor_impl.hpp:128-157,180-248       ICP correspondences+H/b   -> gp_icp_factor_*
//   factors/impl/integrated_loam_factor_impl.hpp:80-194,235-365,444-529   LOAM edge / plane / combined -> gp_loam_factor_*
//
// Nothing of the search lives here: gp::launch_nearest_correspondences (gp_knn.hip) writes, for the source points transformed by the linearisation pose, the index
// of the nearest target point within the cut-off into corr[]; a tile kernel then sums the factor's terms over those correspondences into the partial-row layout of
// the VGICP factor (gp_device.hpp ACC / ACCG), which goes through the same finalize kernels (gp_vgicp_shared.hpp).  The correspondence pass is its own kernel: with
// the search inlined the tile kernel held 157 VGPRs, and measured 0.233 against 0.160 ms per linearise (profiles/r02_gicp_split_ab.jsonl).  The stored
// correspondences are also what the reference's error() evaluates on (it does not search again).
#include "gp_corr_tile.hpp"

namespace gp {

// validate_correspondences of the LOAM factor over the stored correspondences of one part (gp_corr_factors.hpp: loam_validate_point), one point per lane
__global__ void __launch_bounds__(256) loam_validate_kernel(const float* __restrict__ target_points, int* __restrict__ corr, int n, int K) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i < n) loam_validate_point(target_points, corr + i, (size_t)n, K);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

// (the handles: gp_corr_factors.hpp; the tile kernel, the synchronous pass over the stored correspondences and the update rule around it: gp_corr_tile.hpp)

int gp_gicp_factor::run_pass(const double* pose_lin, const double* pose_eval, void* out_host) { return gp_corr_factor_core::run_pass(term, pose_lin, pose_eval, out_host); }

int gp_icp_factor::run_pass(const double* pose_lin, const double* pose_eval, void* out_host) {
  if (plane) return gp_corr_factor_core::run_pass(gp::IcpTerm<true>{desc}, pose_lin, pose_eval, out_host);
  return gp_corr_factor_core::run_pass(gp::IcpTerm<false>{desc}, pose_lin, pose_eval, out_host);
}

int gp_loam_part::run_pass(const double* pose_lin, const double* pose_eval, void* out_host) {
  if (k == 2) return gp_corr_factor_core::run_pass(gp::LoamEdgeTerm{desc}, pose_lin, pose_eval, out_host);
  return gp_corr_factor_core::run_pass(gp::LoamPlaneTerm{desc}, pose_lin, pose_eval, out_host);
}

int gp_loam_part::validate() {
  if (n <= 0) return GP_OK;
  hipLaunchKernelGGL(gp::loam_validate_kernel, dim3((n + 255) / 256), dim3(256), 0, stream, desc.target_points, corr.as<int>(), n, k);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

// ---- LOAM factor: what the entry points share ----

// the searches of both parts at `pose`, with the validation behind them when it is enabled
static int loam_search(gp_loam_factor* f, const double* pose) {
  for (gp_loam_part* p : {f->edge.get(), f->plane.get()})
    if (p && p->num_tiles > 0) GP_TRY(p->search_k(p->k, pose));
  f->upd.note_search(pose);
  return GP_OK;
}

static int loam_validate(gp_loam_factor* f) {
  if (!f->validation) return GP_OK;
  for (gp_loam_part* p : {f->edge.get(), f->plane.get()})
    if (p) GP_TRY(p->validate());
  return GP_OK;
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

int gp_gicp_factor_destroy(gp_gicp_factor_t* f) { return gp_corr_destroy(f); }  // (and its grid)

// (the update rule with zero tolerances: a linearise always searches, an error evaluation at the pose of the last search does not -- gp_corr_tile.hpp)
int gp_gicp_factor_linearize(gp_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_gicp_factor_linearize: null");
  return corr_factor_linearize(f, pose, out_host);
}

int gp_gicp_factor_compute_error(gp_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_gicp_factor_compute_error: null");
  return corr_factor_compute_error(f, pose_lin, pose_eval, out_host);
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

int gp_icp_factor_destroy(gp_icp_factor_t* f) { return gp_corr_destroy(f); }  // (the grid is the caller's)

int gp_icp_factor_set_correspondence_update_tolerance(gp_icp_factor_t* f, double angle, double trans) {
  return gp_corr_set_update_tolerance(f ? &f->upd : nullptr, angle, trans, "gp_icp_factor_set_correspondence_update_tolerance");
}

int gp_icp_factor_num_correspondences(const gp_icp_factor_t* f) { return f ? f->num_inliers : 0; }

int gp_icp_factor_linearize(gp_icp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_linearize: null");
  return corr_factor_linearize(f, pose, out_host);
}

int gp_icp_factor_compute_error(gp_icp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_icp_factor_compute_error: null");
  return corr_factor_compute_error(f, pose_lin, pose_eval, out_host);
}

// ---- LOAM factor ----------------------------------------------------------------------------------------------------

static int loam_make_part(int k, const gp_point_grid_t* grid, const float* target_dev, const float* source_dev, int n, hipStream_t stream, std::unique_ptr<gp_loam_part>* out) {
  auto p = std::make_unique<gp_loam_part>();
  p->k = k;
  p->desc = {source_dev, target_dev};
  GP_TRY(p->prepare(grid, source_dev, n, 1.0, stream));  // max_correspondence_distance_sq(1.0), :27, :205
  GP_TRY(p->corr.alloc(sizeof(int) * (size_t)k * (size_t)std::max(n, 1)));
  *out = std::move(p);
  return GP_OK;
}

int gp_loam_factor_create(const gp_point_grid_t* edge_grid, const float* target_edges_dev, int num_target_edges, const float* source_edges_dev, int num_source_edges,
                          const gp_point_grid_t* plane_grid, const float* target_planes_dev, int num_target_planes, const float* source_planes_dev, int num_source_planes,
                          gp_stream_t stream, gp_loam_factor_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_create: null out");
  *out = nullptr;
  const bool no_edge = !edge_grid && num_target_edges == 0 && num_source_edges == 0, no_plane = !plane_grid && num_target_planes == 0 && num_source_planes == 0;
  if (no_edge && no_plane) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_create: neither an edge part nor a plane part");
  if (!no_edge && (!edge_grid || !target_edges_dev || !source_edges_dev || num_target_edges < 0 || num_source_edges < 0))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_create: the edge part needs its grid, target points and source points");
  if (!no_plane && (!plane_grid || !target_planes_dev || !source_planes_dev || num_target_planes < 0 || num_source_planes < 0))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_create: the plane part needs its grid, target points and source points");
  auto f = std::make_unique<gp_loam_factor>();
  f->stream = (hipStream_t)stream;
  if (!no_edge) GP_TRY(loam_make_part(2, edge_grid, target_edges_dev, source_edges_dev, num_source_edges, f->stream, &f->edge));
  if (!no_plane) GP_TRY(loam_make_part(3, plane_grid, target_planes_dev, source_planes_dev, num_source_planes, f->stream, &f->plane));
  *out = f.release();
  return GP_OK;
}

int gp_loam_factor_destroy(gp_loam_factor_t* f) { return gp_corr_destroy(f); }  // (the grids are the caller's)

int gp_loam_factor_set_max_correspondence_distance(gp_loam_factor_t* f, double dist_edge, double dist_plane) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_set_max_correspondence_distance: null");
  if (!(dist_edge > 0.0) || !(dist_plane > 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_set_max_correspondence_distance: distances must be positive");
  if (f->edge) f->edge->max_sq_dist = dist_edge * dist_edge;
  if (f->plane) f->plane->max_sq_dist = dist_plane * dist_plane;
  return GP_OK;
}

int gp_loam_factor_set_enable_correspondence_validation(gp_loam_factor_t* f, int on) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_set_enable_correspondence_validation: null");
  f->validation = on != 0;
  return GP_OK;
}

int gp_loam_factor_set_correspondence_update_tolerance(gp_loam_factor_t* f, double angle, double trans) {
  return gp_corr_set_update_tolerance(f ? &f->upd : nullptr, angle, trans, "gp_loam_factor_set_correspondence_update_tolerance");
}

int gp_loam_factor_num_correspondences(const gp_loam_factor_t* f, int* edges, int* planes) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_num_correspondences: null");
  if (edges) *edges = f->num_edges;
  if (planes) *planes = f->num_planes;
  return GP_OK;
}

int gp_loam_factor_get_correspondences(const gp_loam_factor_t* f, int* edges_host, int* planes_host) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_get_correspondences: null");
  if (!f->upd.corr_valid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_get_correspondences: no correspondences are stored (never linearised)");
  GP_HIP(hipStreamSynchronize(f->stream));
  if (edges_host && f->edge && f->edge->n > 0) GP_HIP(hipMemcpy(edges_host, f->edge->corr.as<int>(), sizeof(int) * 2 * (size_t)f->edge->n, hipMemcpyDeviceToHost));
  if (planes_host && f->plane && f->plane->n > 0) GP_HIP(hipMemcpy(planes_host, f->plane->corr.as<int>(), sizeof(int) * 3 * (size_t)f->plane->n, hipMemcpyDeviceToHost));
  return GP_OK;
}

// the record of a combined factor: the edge part's finalised record plus the plane part's, added in that order in f64 as IntegratedLOAMFactor_::evaluate does
// (:461-472); a factor of one part hands that part's record on
static void loam_add(const double* edge, const double* plane, double* out, size_t count) {
  for (size_t k = 0; k < count; k++) out[k] = edge && plane ? edge[k] + plane[k] : (edge ? edge[k] : plane[k]);
}

int gp_loam_factor_linearize(gp_loam_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_linearize: null");
  if (!f->upd.keep(pose)) GP_TRY(loam_search(f, pose));
  GP_TRY(loam_validate(f));  // (also behind kept correspondences, as update_correspondences :444-449 does: it is idempotent)
  f->upd.note_linearize(pose);
  gp_linearized6 e{}, p{};
  if (f->edge) GP_TRY(f->edge->run_pass(pose, nullptr, &e));
  if (f->plane) GP_TRY(f->plane->run_pass(pose, nullptr, &p));
  static_assert(sizeof(gp_linearized6) % sizeof(double) == 0, "a record is doubles only");
  loam_add(f->edge ? reinterpret_cast<const double*>(&e) : nullptr, f->plane ? reinterpret_cast<const double*>(&p) : nullptr, reinterpret_cast<double*>(out_host),
           sizeof(gp_linearized6) / sizeof(double));
  f->num_edges = f->edge ? (int)e.num_inliers : 0;
  f->num_planes = f->plane ? (int)p.num_inliers : 0;
  return GP_OK;
}

int gp_loam_factor_compute_error(gp_loam_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_loam_factor_compute_error: null");
  if (!f->upd.stored(pose_lin)) {
    GP_TRY(loam_search(f, pose_lin));
    GP_TRY(loam_validate(f));
  }
  double e = 0.0, p = 0.0;
  if (f->edge) GP_TRY(f->edge->run_pass(pose_lin, pose_eval, &e));
  if (f->plane) GP_TRY(f->plane->run_pass(pose_lin, pose_eval, &p));
  loam_add(f->edge ? &e : nullptr, f->plane ? &p : nullptr, out_host, 1);
  return GP_OK;
}

}  // extern "C"
