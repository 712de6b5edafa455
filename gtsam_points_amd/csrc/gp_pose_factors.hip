// gp_pose_factors.hip -- gtsam::BetweenFactor<Pose3> / gtsam::PriorFactor<Pose3> (Gaussian noise) linearised on the device into gp_linearized6 records, for the dense
// and sparse systems and the device-resident LM graph (gp_lm.hip).  The formulas: gp_pose_factors.hpp.
//
// Kernel shape: one wave per factor (a workgroup of 64 lanes).  A lane per factor would hold J_a, Lambda, Lambda J_a and the 122 outputs at once (~250 f64 values):
// it spills.  Spread over a wave, every lane derives the factor's pose algebra (a few hundred f64 operations, no memory beyond 3 poses), then lanes 0-41 stage
// J_a / Lambda / e in 960 B of LDS and each output double is one lane's fixed-order sum of six products.  The records' bits do not depend on the grid.
#include <cmath>
#include <cstring>

#include "gp_host.hpp"
#include "gp_pose_factors.hpp"
#include "gp_vgicp_shared.hpp"

namespace gp {

__global__ void __launch_bounds__(64) pose_factors_kernel(const gp_pose_factor* __restrict__ factors, int num_factors, const double* __restrict__ poses,
                                                          double* __restrict__ records, double* __restrict__ errors) {
  __shared__ double lds[120];
  const int f = blockIdx.x;
  if (f >= num_factors) return;  // (the whole workgroup: the barriers inside are reached by all of it or none)
  pose_factor_eval(factors[f], poses, lds, records ? records + 122 * (size_t)f : nullptr, errors ? errors + f : nullptr);
}

int check_pose_factors(const gp_pose_factor* factors, int num_factors, int num_poses, const char* api) {
  const std::string a(api);
  if (num_factors < 0 || (num_factors > 0 && !factors) || num_poses < 1) return fail(GP_ERROR_INVALID_ARGUMENT, a + ": factors [num_factors >= 0], num_poses >= 1");
  for (int i = 0; i < num_factors; i++) {
    const gp_pose_factor& f = factors[i];
    const std::string at = a + ": pose factor " + std::to_string(i);
    if (f.kind != GP_POSE_FACTOR_BETWEEN && f.kind != GP_POSE_FACTOR_PRIOR) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": unknown kind");
    if (f.pose_a < 0 || f.pose_a >= num_poses) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": pose_a out of range");
    if (f.kind == GP_POSE_FACTOR_BETWEEN) {
      if (f.pose_b < 0 || f.pose_b >= num_poses) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": pose_b out of range");
      if (f.pose_b == f.pose_a) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": a between factor of a pose and itself");
    } else if (f.pose_b != -1) {
      return fail(GP_ERROR_INVALID_ARGUMENT, at + ": a prior has pose_b = -1");
    }
    if (!pose_is_rigid(f.measured)) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": measured is not a rigid transform (orthonormal to 1e-9, det > 0)");
    double scale = 0.0;
    for (int k = 0; k < 36; k++) {
      if (!std::isfinite(f.information[k])) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": information is not finite");
      scale = std::fmax(scale, std::fabs(f.information[k]));
    }
    for (int r = 0; r < 6; r++)
      for (int c = r + 1; c < 6; c++)
        if (!(std::fabs(f.information[c * 6 + r] - f.information[r * 6 + c]) <= 1e-12 * scale)) return fail(GP_ERROR_INVALID_ARGUMENT, at + ": information is not symmetric");
  }
  return GP_OK;
}

int launch_pose_factors(const gp_pose_factor* factors_dev, int num_factors, const double* poses_dev, gp_linearized6* records, double* errors, hipStream_t stream) {
  if (num_factors <= 0) return GP_OK;
  hipLaunchKernelGGL(pose_factors_kernel, dim3((unsigned)num_factors), dim3(64), 0, stream, factors_dev, num_factors, poses_dev, reinterpret_cast<double*>(records), errors);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

}  // namespace gp

struct gp_pose_factors {
  hipStream_t stream = nullptr;
  int P = 0, N = 0;
  gp::DeviceArray d_factors, d_poses, d_out;
};

extern "C" {

int gp_pose_factors_create(const gp_pose_factor* factors, int num_factors, int num_poses, gp_stream_t stream, gp_pose_factors_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_pose_factors_create: null out");
  *out = nullptr;
  GP_TRY(gp::check_pose_factors(factors, num_factors, num_poses, "gp_pose_factors_create"));
  auto* pf = new gp_pose_factors;
  pf->stream = (hipStream_t)stream, pf->P = num_factors, pf->N = num_poses;
  int rc = pf->d_factors.alloc(sizeof(gp_pose_factor) * (size_t)num_factors);
  if (rc == GP_OK && num_factors > 0 && hipMemcpy(pf->d_factors.ptr, factors, sizeof(gp_pose_factor) * (size_t)num_factors, hipMemcpyHostToDevice) != hipSuccess)
    rc = gp::fail(GP_ERROR_HIP, "gp_pose_factors_create: upload of the factors");
  if (rc != GP_OK) {
    delete pf;
    return rc;
  }
  *out = pf;
  return GP_OK;
}

int gp_pose_factors_destroy(gp_pose_factors_t* pf) {
  if (!pf) return GP_OK;
  (void)hipStreamSynchronize(pf->stream);
  delete pf;
  return GP_OK;
}

int gp_pose_factors_size(const gp_pose_factors_t* pf) { return pf ? pf->P : 0; }

int gp_pose_factors_issue_linearize_dev(gp_pose_factors_t* pf, const double* poses_dev, gp_linearized6* out_dev) {
  if (!pf || !poses_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_pose_factors_issue_linearize_dev: null");
  return gp::launch_pose_factors(pf->d_factors.as<gp_pose_factor>(), pf->P, poses_dev, out_dev, nullptr, pf->stream);
}

int gp_pose_factors_issue_compute_error_dev(gp_pose_factors_t* pf, const double* poses_dev, double* out_dev) {
  if (!pf || !poses_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_pose_factors_issue_compute_error_dev: null");
  return gp::launch_pose_factors(pf->d_factors.as<gp_pose_factor>(), pf->P, poses_dev, nullptr, out_dev, pf->stream);
}

// the synchronous forms: poses up, one launch, results down, one wait
static int run_sync(gp_pose_factors_t* pf, const double* poses_host, void* out_host, bool records, const char* api) {
  if (!pf || !poses_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, std::string(api) + ": null");
  const size_t out_bytes = (records ? sizeof(gp_linearized6) : sizeof(double)) * (size_t)pf->P;
  GP_TRY(pf->d_poses.ensure(sizeof(double) * 16 * (size_t)pf->N));
  GP_TRY(pf->d_out.ensure(out_bytes));
  GP_HIP(hipMemcpyAsync(pf->d_poses.ptr, poses_host, sizeof(double) * 16 * (size_t)pf->N, hipMemcpyHostToDevice, pf->stream));
  GP_TRY(gp::launch_pose_factors(pf->d_factors.as<gp_pose_factor>(), pf->P, pf->d_poses.as<double>(), records ? pf->d_out.as<gp_linearized6>() : nullptr,
                                 records ? nullptr : pf->d_out.as<double>(), pf->stream));
  if (out_bytes) GP_HIP(hipMemcpyAsync(out_host, pf->d_out.ptr, out_bytes, hipMemcpyDeviceToHost, pf->stream));
  GP_HIP(hipStreamSynchronize(pf->stream));
  return GP_OK;
}

int gp_pose_factors_linearize(gp_pose_factors_t* pf, const double* poses_host, gp_linearized6* out_host) { return run_sync(pf, poses_host, out_host, true, "gp_pose_factors_linearize"); }

int gp_pose_factors_compute_error(gp_pose_factors_t* pf, const double* poses_host, double* out_host) { return run_sync(pf, poses_host, out_host, false, "gp_pose_factors_compute_error"); }

}  // extern "C"
