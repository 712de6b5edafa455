// gp_color_consistency.hip -- the color consistency factor on nearest-neighbour correspondences: the purely photometric matching cost.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/impl/integrated_color_consistency_factor_impl.hpp:101-253    correspondences + H/b    -> gp_color_consistency_factor_*
//
// One more term on the correspondence core (gp_corr_tile.hpp): gp_corr_factor_core::search writes the nearest target point of every source point -- in 3-D on a
// gp_point_grid, or in (x, y, z, intensity) on a gp_intensity_grid (gp_intensity_search.hip) --, the tile kernel sums ColorConsistencyTerm (gp_colored_term.hpp) over
// them through accumulate_sums_mw into the partial-row layout of the VGICP factor, the VGICP finalize kernels expand the rows.
#include <cmath>

#include "gp_colored_term.hpp"
#include "gp_corr_tile.hpp"

int gp_color_consistency_factor::run_pass(const double* pose_lin, const double* pose_eval, void* out_host) {
  return gp_corr_factor_core::run_pass(term, pose_lin, pose_eval, out_host);
}

extern "C" {

int gp_color_consistency_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_normals_dev, const float* target_intensities_dev,
                                       const float* target_gradients_dev, int n_target, const float* points_dev, const float* intensities_dev, int n,
                                       double max_correspondence_distance_sq, double photometric_term_weight, gp_stream_t stream, gp_color_consistency_factor_t** out) {
  // (an EMPTY source may come with NULL arrays -- an empty device tensor has no address --: its record is the zero record, nothing is ever read)
  if (!grid || !target_points_dev || !target_normals_dev || !target_intensities_dev || !target_gradients_dev || (n != 0 && (!points_dev || !intensities_dev)) || n < 0 ||
      n_target < 0 || !(max_correspondence_distance_sq > 0.0) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_create: bad arguments (a NULL grid or array, a negative count, a cut-off that is not positive)");
  if (!(photometric_term_weight >= 0.0) || !std::isfinite(photometric_term_weight))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_create: photometric_term_weight negative or not finite");
  auto f = std::make_unique<gp_color_consistency_factor>();
  f->term = {points_dev, intensities_dev, target_points_dev, target_normals_dev, target_intensities_dev, target_gradients_dev, photometric_term_weight};
  GP_TRY(f->prepare(grid, points_dev, n, max_correspondence_distance_sq, (hipStream_t)stream));
  *out = f.release();
  return GP_OK;
}

int gp_color_consistency_factor_destroy(gp_color_consistency_factor_t* f) { return gp_corr_destroy(f); }  // (the grids are the caller's)

int gp_color_consistency_factor_set_intensity_grid(gp_color_consistency_factor_t* f, const gp_intensity_grid_t* xyzi) {
  return gp_corr_set_intensity_grid(f, xyzi, f ? f->term.intensities : nullptr, "gp_color_consistency_factor_set_intensity_grid");
}

int gp_color_consistency_factor_set_photometric_term_weight(gp_color_consistency_factor_t* f, double weight) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_set_photometric_term_weight: null");
  if (!(weight >= 0.0) || !std::isfinite(weight))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_set_photometric_term_weight: weight negative or not finite");
  f->term.photometric_term_weight = weight;
  return GP_OK;
}

int gp_color_consistency_factor_set_max_correspondence_distance(gp_color_consistency_factor_t* f, double dist) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_set_max_correspondence_distance: null");
  if (!(dist > 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_set_max_correspondence_distance: the distance must be positive");
  f->max_sq_dist = dist * dist;
  return GP_OK;
}

int gp_color_consistency_factor_set_correspondence_update_tolerance(gp_color_consistency_factor_t* f, double angle, double trans) {
  return gp_corr_set_update_tolerance(f ? &f->upd : nullptr, angle, trans, "gp_color_consistency_factor_set_correspondence_update_tolerance");
}

int gp_color_consistency_factor_num_correspondences(const gp_color_consistency_factor_t* f) { return f ? f->num_inliers : 0; }

int gp_color_consistency_factor_linearize(gp_color_consistency_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_linearize: null");
  return corr_factor_linearize(f, pose, out_host);
}

int gp_color_consistency_factor_compute_error(gp_color_consistency_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_color_consistency_factor_compute_error: null");
  return corr_factor_compute_error(f, pose_lin, pose_eval, out_host);
}

}  // extern "C"
