// gp_colored_factors.hip -- the colored GICP factor on nearest-neighbour correspondences and the intensity gradients it reads.
//
// Replaces (reference, CPU only -- there is no GPU counterpart upstream):
//   factors/intensity_gradients.cpp:20-133                               IntensityGradients::estimate  -> gp_estimate_intensity_gradients*
//   factors/impl/integrated_colored_gicp_factor_impl.hpp:101-253         correspondences + H/b         -> gp_colored_gicp_factor_*
//
// The factor is one more term on the correspondence core (gp_corr_tile.hpp): gp::launch_nearest_correspondences writes the nearest target point of every source
// point, the tile kernel sums the term over them into the partial-row layout of the VGICP factor (gp_device.hpp ACC / ACCG), the VGICP finalize kernels expand
// the rows.  The one difference to the other terms is that the photometric residual adds a rank-one part to both M and the right-hand side, so the sums are fed
// with (M, w, error) instead of (M, d): see accumulate_sums_mw (gp_colored_term.hpp, where the term lives: the correspondence batch instantiates it too).
#include <limits>

#include "gp_colored_term.hpp"
#include "gp_corr_tile.hpp"

namespace gp {

// IntensityGradients::estimate (intensity_gradients.cpp:40-66), one point per lane, f64 on the f32 inputs: rows of A are the normal (b = 0) and, for the slots
// 1 .. k_photo - 1 of the point's neighbour list (slot 0 is the point itself and is skipped, :54), the neighbour projected onto the tangent plane minus the point
// with b = I_j - I; H = A^T A, e = A^T b, g = H^-1 e with the cofactor inverse, rounded once at the store.  The hot part is the gather of k_photo x 16 B.
// A slot among the first k_photo that is no point index (the search's -1 padding; anything outside [0, n) is refused the same way) gives (0, 0, 0) and counts
// in *num_short.  A singular H is not guarded: its non-finite values are stored.
__global__ void __launch_bounds__(256) intensity_gradient_kernel(const float* __restrict__ points, const float* __restrict__ normals, const float* __restrict__ intensities,
                                                                 int n, const int* __restrict__ neighbors, int k, int k_photo, float* __restrict__ gradients,
                                                                 int* __restrict__ num_short) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int* __restrict__ nb = neighbors + (size_t)i * (size_t)k;
  bool ok = true;
  for (int j = 0; j < k_photo; j++) ok = ok && (unsigned)nb[j] < (unsigned)n;
  float* __restrict__ out = gradients + 3 * (size_t)i;
  if (!ok) {
    out[0] = out[1] = out[2] = 0.0f;
    if (num_short) atomicAdd(num_short, 1);
    return;
  }
  const double px = (double)points[3 * (size_t)i], py = (double)points[3 * (size_t)i + 1], pz = (double)points[3 * (size_t)i + 2];
  const double nx = (double)normals[3 * (size_t)i], ny = (double)normals[3 * (size_t)i + 1], nz = (double)normals[3 * (size_t)i + 2];
  const double intensity = (double)intensities[i];
  double h00 = nx * nx, h01 = nx * ny, h02 = nx * nz, h11 = ny * ny, h12 = ny * nz, h22 = nz * nz;  // row 0 of A: the normal
  double e0 = 0.0, e1 = 0.0, e2 = 0.0;
  for (int j = 1; j < k_photo; j++) {
    const size_t t = (size_t)nb[j];
    const double tx = (double)points[3 * t], ty = (double)points[3 * t + 1], tz = (double)points[3 * t + 2];
    const double b = (double)intensities[t] - intensity;
    const double along = (tx - px) * nx + (ty - py) * ny + (tz - pz) * nz;
    const double ax = (tx - along * nx) - px, ay = (ty - along * ny) - py, az = (tz - along * nz) - pz;
    h00 += ax * ax;
    h01 += ax * ay;
    h02 += ax * az;
    h11 += ay * ay;
    h12 += ay * az;
    h22 += az * az;
    e0 += ax * b;
    e1 += ay * b;
    e2 += az * b;
  }
  double hi[6];
  inverse_sym3(h00, h01, h02, h11, h12, h22, hi);
  out[0] = (float)(hi[0] * e0 + hi[1] * e1 + hi[2] * e2);
  out[1] = (float)(hi[1] * e0 + hi[3] * e1 + hi[4] * e2);
  out[2] = (float)(hi[2] * e0 + hi[4] * e1 + hi[5] * e2);
}

}  // namespace gp

// ---------------------------------------------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------------------------------------------

int gp_colored_gicp_factor::run_pass(const double* pose_lin, const double* pose_eval, void* out_host) {
  return gp_corr_factor_core::run_pass(term, pose_lin, pose_eval, out_host);
}

extern "C" {

// ---- intensity gradients ----------------------------------------------------------------------------------------------

int gp_estimate_intensity_gradients_from_neighbors(const float* points_dev, const float* normals_dev, const float* intensities_dev, int n, const int* neighbors_dev, int k,
                                                   int k_photo, float* gradients_dev, gp_stream_t stream) {
  if (!points_dev || !normals_dev || !intensities_dev || !neighbors_dev || !gradients_dev || n < 0 || k < 1 || k_photo < 1 || k_photo > k)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_intensity_gradients_from_neighbors: bad arguments (no NULL array, n >= 0, 1 <= k_photo <= k)");
  if (n == 0) return GP_OK;
  hipLaunchKernelGGL(gp::intensity_gradient_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, points_dev, normals_dev, intensities_dev, n, neighbors_dev, k,
                     k_photo, gradients_dev, static_cast<int*>(nullptr));
  GP_HIP(hipGetLastError());
  return GP_OK;
}

int gp_estimate_intensity_gradients(const float* points_dev, const float* normals_dev, const float* intensities_dev, int n, int k, double cell_size, float* gradients_dev,
                                    int* num_short, gp_stream_t stream) {
  if (!points_dev || !normals_dev || !intensities_dev || !gradients_dev || n < 0 || k < 1 || k > 32)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_estimate_intensity_gradients: bad arguments (no NULL array, n >= 0, 1 <= k <= 32)");
  if (num_short) *num_short = 0;
  if (n == 0) return GP_OK;
  hipStream_t s = (hipStream_t)stream;
  struct Grid {
    gp_point_grid_t* g = nullptr;
    ~Grid() {
      if (g) gp_point_grid_destroy(g);
    }
  } grid;
  GP_TRY(gp_point_grid_create(points_dev, n, cell_size > 0.0 ? cell_size : 0.25, stream, &grid.g));
  gp::DeviceArray table, counter;  // int[n][k] neighbour lists; the number of points with fewer than k
  GP_TRY(table.alloc_async(sizeof(int) * (size_t)n * (size_t)k, s));
  GP_TRY(counter.alloc_async(sizeof(int), s));
  GP_HIP(hipMemsetAsync(counter.ptr, 0, sizeof(int), s));
  GP_TRY(gp_knn_search(grid.g, points_dev, n, k, std::numeric_limits<double>::max(), table.as<int>(), nullptr, nullptr, stream));
  hipLaunchKernelGGL(gp::intensity_gradient_kernel, dim3((n + 255) / 256), dim3(256), 0, s, points_dev, normals_dev, intensities_dev, n, table.as<int>(), k, k, gradients_dev,
                     counter.as<int>());
  GP_HIP(hipGetLastError());
  int h_short = 0;
  GP_HIP(hipMemcpyAsync(&h_short, counter.ptr, sizeof(int), hipMemcpyDeviceToHost, s));
  GP_HIP(hipStreamSynchronize(s));  // (also: the search has finished with the grid before it goes)
  if (num_short) *num_short = h_short;
  return GP_OK;
}

// ---- colored GICP factor ----------------------------------------------------------------------------------------------

int gp_colored_gicp_factor_create(const gp_point_grid_t* grid, const float* target_points_dev, const float* target_covs_dev, const float* target_normals_dev,
                                  const float* target_intensities_dev, const float* target_gradients_dev, int n_target, const float* points_dev, const float* covs_dev,
                                  const float* intensities_dev, int n, double max_correspondence_distance_sq, double photometric_term_weight, gp_stream_t stream,
                                  gp_colored_gicp_factor_t** out) {
  if (!grid || !target_points_dev || !target_covs_dev || !target_normals_dev || !target_intensities_dev || !target_gradients_dev || !points_dev || !covs_dev ||
      !intensities_dev || n < 0 || n_target < 0 || !(max_correspondence_distance_sq > 0.0) || !out)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_create: bad arguments (a NULL grid or array, a negative count, a cut-off that is not positive)");
  if (!(photometric_term_weight >= 0.0 && photometric_term_weight <= 1.0))
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_create: photometric_term_weight outside [0, 1]");
  auto f = std::make_unique<gp_colored_gicp_factor>();
  f->term = {points_dev,         covs_dev,        intensities_dev,       target_points_dev, target_covs_dev, target_normals_dev, target_intensities_dev,
             target_gradients_dev, photometric_term_weight};
  GP_TRY(f->prepare(grid, points_dev, n, max_correspondence_distance_sq, (hipStream_t)stream));
  *out = f.release();
  return GP_OK;
}

int gp_colored_gicp_factor_destroy(gp_colored_gicp_factor_t* f) { return gp_corr_destroy(f); }  // (the grid is the caller's)

int gp_colored_gicp_factor_set_intensity_grid(gp_colored_gicp_factor_t* f, const gp_intensity_grid_t* xyzi) {
  return gp_corr_set_intensity_grid(f, xyzi, f ? f->term.intensities : nullptr, "gp_colored_gicp_factor_set_intensity_grid");
}

int gp_colored_gicp_factor_set_photometric_term_weight(gp_colored_gicp_factor_t* f, double weight) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_photometric_term_weight: null");
  if (!(weight >= 0.0 && weight <= 1.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_photometric_term_weight: weight outside [0, 1]");
  f->term.photometric_term_weight = weight;
  return GP_OK;
}

int gp_colored_gicp_factor_set_max_correspondence_distance(gp_colored_gicp_factor_t* f, double dist) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_max_correspondence_distance: null");
  if (!(dist > 0.0)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_set_max_correspondence_distance: the distance must be positive");
  f->max_sq_dist = dist * dist;
  return GP_OK;
}

int gp_colored_gicp_factor_set_correspondence_update_tolerance(gp_colored_gicp_factor_t* f, double angle, double trans) {
  return gp_corr_set_update_tolerance(f ? &f->upd : nullptr, angle, trans, "gp_colored_gicp_factor_set_correspondence_update_tolerance");
}

int gp_colored_gicp_factor_num_correspondences(const gp_colored_gicp_factor_t* f) { return f ? f->num_inliers : 0; }

int gp_colored_gicp_factor_linearize(gp_colored_gicp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_linearize: null");
  return corr_factor_linearize(f, pose, out_host);
}

int gp_colored_gicp_factor_compute_error(gp_colored_gicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_colored_gicp_factor_compute_error: null");
  return corr_factor_compute_error(f, pose_lin, pose_eval, out_host);
}

}  // extern "C"
