// gp_vgicp_batch.hip -- the entry points of the VGICP path that the product calls: gp_vgicp_factor_* and gp_vgicp_batch_*.  What they stand on: tables, tuning and pose
// staging are gp_vgicp_table.hip, the arrival protocol of the fused finalize is gp_vgicp_arrival.hpp, the kernels and their launches gp_vgicp.hip; the check hooks
// and the measurement entry points are gp_vgicp_debug.hip.  The units share gp_vgicp_batch.hpp.
//
// Replaces (reference): the per-factor launch loop of src/gtsam_points/cuda/nonlinear_factor_set_gpu.cpp:64-218.
#include <algorithm>
#include <cstring>

#include "gp_host.hpp"
#include "gp_vgicp_arrival.hpp"
#include "gp_vgicp_batch.hpp"

using gp::Arrival;
using gp::ensure_self_batch;
using gp::ensure_table;
using gp::finish_fused;
using gp::launch_error;
using gp::PoseSource;
using gp::takes_rigid_path;

constexpr size_t kRecordDoubles = sizeof(gp_linearized6) / sizeof(double);

// the step of a by-part fused linearise as the device saw it: first workgroup started .. last row in .. last sums out (words 34 / 32 / 33 of the parts' slots)
static void read_device_stamps(gp_vgicp_batch_t* b, int parts) {
  const unsigned long long* w = static_cast<const unsigned long long*>(b->h_out.ptr);
  unsigned long long t0 = ~0ull, t_rows = 0, t_out = 0;
  for (int g = 0; g < parts; g++) {
    if (g < gp::kNumXCD) t0 = std::min(t0, w[g * kRecordDoubles + 34]);
    t_rows = std::max(t_rows, w[g * kRecordDoubles + 32]);
    t_out = std::max(t_out, w[g * kRecordDoubles + 33]);
  }
  if (t0 <= t_rows && t_rows <= t_out && t_out - t0 < 100000000ull) {
    b->measurement.dev_steps += 1.0;
    b->measurement.dev_stream_ticks += (double)(t_rows - t0);
    b->measurement.dev_kernel_ticks += (double)(t_out - t0);
  }
}

// synchronous: the finalize kernel stores the records straight into host-mapped pinned memory (no D2H copy op).
// out_host != nullptr: the records are copied there; view != nullptr: *view points at them where they lie (the batch's own pinned
// buffer, or `view_store` for the single large factor whose parts the host combines) until the next call on the batch.
static int batch_linearize_sync(gp_vgicp_batch_t* b, const double* poses_host, gp_linearized6* out_host, const gp_linearized6** view) {
  const size_t F = b->factors.size();
  if (view) *view = nullptr;
  if (F == 0) return GP_OK;
  gp_linearized6 local;
  if (!out_host && F == 1) out_host = view ? &b->view_store : &local;  // (the combined record of a split finalize needs a home)
  GP_TRY(ensure_table(b));
  PoseSource ps;
  GP_TRY(gp::stage_poses(b, poses_host, nullptr, &ps, true));
  const gp::DoneFlags done = gp::next_done(b, b->trace ? b->trace + 2047 * 16 : nullptr);
  const bool rigid = takes_rigid_path(b, poses_host);
  const int parts = gp::linearize_parts(b, rigid);
  const bool sums_only = parts > 1;  // the parts deliver their 32 sums, the host expands once (the parts expanding: measured slower, round 2)
  const bool timing = b->measurement.timing;
  if (timing && !b->ev[0])
    for (auto& e : b->ev) GP_HIP(hipEventCreate(&e));
  const bool may_fuse = b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !timing;
  gp_linearized6* const records = reinterpret_cast<gp_linearized6*>(b->h_out_dev);
  double* partials = nullptr;
  if (may_fuse && sums_only && ps.inl.use) {
    // ONE launch: the last workgroup of each part of the tile list finalizes the part; if its word is missing, the finalize kernel does this call's sums
    bool recovered = false;
    GP_TRY(gp::launch_fused_parts<gp::MODE_LIN>(b, &ps, parts, done, &partials));
    GP_TRY(finish_fused(
        b, Arrival::by_part, (size_t)parts, done.seq, false, [&](const gp::DoneFlags& again) { return gp::launch_finalize<false>(b, ps, partials, records, again, -parts); },
        &recovered));
    if (!recovered) read_device_stamps(b, parts);
  } else if (may_fuse && parts == 1 && rigid && !b->trace) {
    // ONE launch for a batch (or a small single factor): the workgroup that stores a factor's last row finalizes the factor, so the records leave for the host
    // while the other factors' tiles are still running; if a word is missing, the finalize kernel does this call's records
    GP_TRY(gp::launch_fused_factors<gp::MODE_LIN>(b, &ps, poses_host, done, &partials));
    GP_TRY(finish_fused(b, Arrival::by_factor, F, done.seq, false, [&](const gp::DoneFlags& again) {
      ps.inl.arrive = nullptr;
      return gp::launch_finalize<false>(b, ps, partials, records, again, 1);
    }));
  } else {
    GP_TRY(gp::launch_linearize(b, ps, records, rigid, done, sums_only ? -parts : parts, timing));
    GP_TRY(gp::wait_words(b, F * (size_t)parts, done.seq));
  }
  if (timing) {  // measurement: the two kernels of THIS synchronous pass, i.e. behind the idle queue the host left between two passes
    GP_HIP(hipEventSynchronize(b->ev[2]));
    GP_HIP(hipEventElapsedTime(&b->measurement.last_tile_ms, b->ev[0], b->ev[1]));
    GP_HIP(hipEventElapsedTime(&b->measurement.last_finalize_ms, b->ev[1], b->ev[2]));
  }
  if (parts == 1) {
    if (view) *view = static_cast<const gp_linearized6*>(b->h_out.ptr);
    if (out_host && !(view && F == 1)) memcpy(out_host, b->h_out.ptr, sizeof(gp_linearized6) * F);
  } else {
    if (view) *view = out_host;  // F == 1: caller's array or view_store
    const double* p = static_cast<const double*>(b->h_out.ptr);
    // the parts' 32 sums add up in slot order; one expansion on the host
    double total[32];
    for (int k = 0; k < 32; k++) {
      double a = p[k];
      for (int q = 1; q < parts; q++) a += p[(size_t)q * kRecordDoubles + k];
      total[k] = a;
    }
    gp::expand_rigid_host(total, poses_host, reinterpret_cast<double*>(out_host));
  }
  return GP_OK;
}

extern "C" {

int gp_vgicp_batch_set_tuning(gp_vgicp_batch_t* b, int key, int value) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_set_tuning: null batch");
  if (key == GP_TUNE_TIMING) {
    b->measurement.timing = value != 0;
    return GP_OK;
  }
  if (key == GP_TUNE_TEST_ARRIVAL_SKEW) {  // test hook: the host's idea of arrival counter 0 runs `value` ahead of the device's, as after a launch that was lost
    b->arrival.arrived[0] += (unsigned long long)(value > 0 ? value : 0);
    if (b->arrival.d_factor_arrive.ptr && value > 0) {  // ... and factor counter 0 is far out of range: that factor's record cannot complete
      const unsigned long long v = 1ull << 40;
      GP_HIP(hipStreamSynchronize(b->stream));
      GP_HIP(hipMemcpy(b->arrival.d_factor_arrive.ptr, &v, sizeof(v), hipMemcpyHostToDevice));
    }
    return GP_OK;
  }
  GP_TRY(gp::apply_tuning(&b->tuning, key, value));
  b->table_dirty = true;
  return GP_OK;
}

int gp_vgicp_batch_get_tuning(const gp_vgicp_batch_t* b, int key, int* value) {
  if (!b || !value) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_get_tuning: null");
  if (key == GP_TUNE_EFFECTIVE_KERNEL) {  // what the last table build resolved GP_TUNE_KERNEL to
    *value = b->table_dirty ? -1 : b->family;
  } else if (key == GP_TUNE_EFFECTIVE_MIRROR) {  // does the built table stream the packed mirrors?
    *value = b->table_dirty ? -1 : (b->packed ? 1 : 0);
  } else if (!gp::read_tuning(b->tuning, key, value)) {
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "unknown GP_TUNE_* key");
  }
  return GP_OK;
}

// the per-factor entry points run a batch of one: its tuning is the factor's
int gp_vgicp_factor_set_tuning(gp_vgicp_factor_t* f, int key, int value) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_set_tuning: null factor");
  GP_TRY(gp::apply_tuning(&f->tuning, key, value));
  if (f->self_batch) {
    f->self_batch->tuning = f->tuning;
    f->self_batch->table_dirty = true;
  }
  return GP_OK;
}

size_t gp_vgicp_linearization_input_size(void) { return sizeof(double) * 16; }
size_t gp_vgicp_linearization_output_size(void) { return sizeof(gp_linearized6); }
size_t gp_vgicp_evaluation_input_size(void) { return sizeof(double) * 16; }
size_t gp_vgicp_evaluation_output_size(void) { return sizeof(double); }

int gp_vgicp_factor_create(const gp_voxelmap_t* target, const float* points_dev, const float* covs_dev, const float* normals_dev, int num_points,
                           gp_stream_t stream, gp_temp_buffer_t* temp_buffer, gp_vgicp_factor_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_create: null out");
  // the reference abort()s on these (integrated_vgicp_factor_gpu.cpp:33-46); the C++ mirror keeps that, the C-ABI reports
  if (!points_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "error: GPU source points have not been allocated!!");
  if (!covs_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "error: GPU source covs have not been allocated!!");
  if (!target) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "error: GPU target voxels have not been created!!");
  if (num_points < 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_create: negative size");
  auto* f = new gp_vgicp_factor;
  f->target = target;
  f->points = points_dev;
  f->covs = covs_dev;
  f->normals = normals_dev;
  f->n = num_points;
  {
    hipPointerAttribute_t attr{};
    int cur = 0;
    (void)hipGetDevice(&cur);
    f->device = (hipPointerGetAttributes(&attr, points_dev) == hipSuccess) ? attr.device : cur;
    (void)hipGetLastError();  // a pointer the runtime does not know leaves a sticky error behind
  }
  if (stream) {
    f->stream = (hipStream_t)stream;
  } else {
    hipError_t e = hipStreamCreateWithFlags(&f->stream, hipStreamNonBlocking);  // integrated_vgicp_derivatives.cu:36-39
    if (e != hipSuccess) {
      delete f;
      return gp::hip_fail(e, "hipStreamCreateWithFlags", __FILE__, __LINE__);
    }
    f->owns_stream = true;
  }
  if (temp_buffer) {
    f->temp_buffer = temp_buffer;
  } else {
    int rc = gp_temp_buffer_create(0, &f->temp_buffer);  // :41-43
    if (rc != GP_OK) {
      if (f->owns_stream) (void)hipStreamDestroy(f->stream);
      delete f;
      return rc;
    }
    f->owns_temp_buffer = true;
  }
  *out = f;
  return GP_OK;
}

int gp_vgicp_factor_destroy(gp_vgicp_factor_t* f) {
  if (!f) return GP_OK;
  if (f->self_batch) gp_vgicp_batch_destroy(f->self_batch);
  if (f->owns_stream) {
    (void)hipStreamSynchronize(f->stream);
    (void)hipStreamDestroy(f->stream);
  }
  if (f->owns_temp_buffer) gp_temp_buffer_destroy(f->temp_buffer);
  delete f;
  return GP_OK;
}

int gp_vgicp_factor_set_surface_validation(gp_vgicp_factor_t* f, int enable) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "null factor");
  if (enable && !f->normals) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "surface validation needs source normals (integrated_vgicp_factor_gpu.hpp:84-86)");
  f->surface_validation = enable != 0;
  f->generation++;
  return GP_OK;
}

// the source cloud was offloaded and reloaded (PointCloudGPU::reload_gpu re-allocates): hand the factor the new arrays
int gp_vgicp_factor_set_source(gp_vgicp_factor_t* f, const float* points_dev, const float* covs_dev, const float* normals_dev) {
  if (!f || !points_dev || !covs_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_set_source: null factor / points / covs");
  if (f->surface_validation && !normals_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_set_source: surface validation is on but no normals given");
  f->points = points_dev;
  f->covs = covs_dev;
  f->normals = normals_dev;
  f->mirror.reset();  // (also the way to say "the arrays were rewritten in place": the next table build packs afresh, or joins the mirror of the new arrays)
  f->mirror_tried = false;
  f->generation++;
  return GP_OK;
}

int gp_vgicp_factor_set_inlier_update_thresh(gp_vgicp_factor_t* f, double trans, double angle) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "null factor");
  f->inlier_thresh_trans = trans;
  f->inlier_thresh_angle = angle;
  return GP_OK;
}

int gp_vgicp_factor_num_points(const gp_vgicp_factor_t* f) { return f ? f->n : 0; }
int gp_vgicp_factor_device(const gp_vgicp_factor_t* f) { return f ? f->device : 0; }
gp_stream_t gp_vgicp_factor_stream(const gp_vgicp_factor_t* f) { return f ? (gp_stream_t)f->stream : nullptr; }

int gp_vgicp_factor_issue_linearize(gp_vgicp_factor_t* f, const double* pose_host, const double* pose_dev, gp_linearized6* out_dev) {
  if (!f || (!pose_dev && !pose_host) || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_issue_linearize: null");
  GP_TRY(ensure_self_batch(f));
  PoseSource ps;
  if (pose_host) gp::inline_poses(f->self_batch, pose_host, nullptr, &ps);  // the host copy rides in the kernel arguments; the device copy is not even read
  else ps = gp::device_poses(pose_dev);
  return gp::launch_linearize(f->self_batch, ps, out_dev, takes_rigid_path(f->self_batch, pose_host));
}

int gp_vgicp_factor_issue_compute_error(gp_vgicp_factor_t* f, const double* pose_lin_host, const double* pose_eval_host, const double* pose_lin_dev,
                                        const double* pose_eval_dev, double* out_dev) {
  if (!f || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_issue_compute_error: null");
  GP_TRY(ensure_self_batch(f));
  PoseSource ps;
  if (pose_lin_host && pose_eval_host) {
    gp::inline_poses(f->self_batch, pose_lin_host, pose_eval_host, &ps);
  } else if (pose_lin_dev && pose_eval_dev) {
    ps = gp::device_poses(pose_lin_dev, pose_eval_dev);
  } else {
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_issue_compute_error: poses missing");
  }
  return launch_error(f->self_batch, ps, out_dev);
}

int gp_vgicp_factor_sync(gp_vgicp_factor_t* f) {
  if (!f) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "null factor");
  GP_HIP(hipStreamSynchronize(f->stream));
  return GP_OK;
}

int gp_vgicp_factor_linearize(gp_vgicp_factor_t* f, const double pose[16], gp_linearized6* out_host) {
  if (!f || !pose || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_linearize: null");
  GP_TRY(ensure_self_batch(f));
  return gp_vgicp_batch_linearize(f->self_batch, pose, out_host);
}

int gp_vgicp_factor_compute_error(gp_vgicp_factor_t* f, const double pose_lin[16], const double pose_eval[16], double* out_host) {
  if (!f || !pose_lin || !pose_eval || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_compute_error: null");
  GP_TRY(ensure_self_batch(f));
  return gp_vgicp_batch_compute_error(f->self_batch, pose_lin, pose_eval, out_host);
}

// ---- batch ----------------------------------------------------------------------------------------------------

int gp_vgicp_batch_create(gp_vgicp_factor_t* const* factors, int num_factors, gp_stream_t stream, gp_vgicp_batch_t** out) {
  if (!out || num_factors < 0 || (num_factors > 0 && !factors)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_create: bad arguments");
  auto* b = new gp_vgicp_batch;
  for (int i = 0; i < num_factors; i++) {
    if (!factors[i]) {
      delete b;
      return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_create: null factor");
    }
    b->factors.push_back(factors[i]);
  }
  b->stream = (hipStream_t)stream;
  int rc = gp::build_table(b);
  if (rc != GP_OK) {
    delete b;
    return rc;
  }
  *out = b;
  return GP_OK;
}

int gp_vgicp_batch_destroy(gp_vgicp_batch_t* batch) {
  if (!batch) return GP_OK;
  for (auto& e : batch->ev)
    if (e) (void)hipEventDestroy(e);
  // the staging buffers are about to be freed: the last H2D copy must have finished.  The stream itself is the caller's and may
  // already be gone (the reference's clone() drops it, integrated_vgicp_factor_gpu.cpp:122-134), so it is not synchronised here.
  if (batch->h2d_done) {
    (void)hipEventSynchronize(batch->h2d_done);
    (void)hipEventDestroy(batch->h2d_done);
  }
  delete batch;
  return GP_OK;
}

int gp_vgicp_batch_size(const gp_vgicp_batch_t* batch) { return batch ? (int)batch->factors.size() : 0; }
int64_t gp_vgicp_batch_total_points(const gp_vgicp_batch_t* batch) { return batch ? batch->total_points : 0; }

int gp_vgicp_batch_issue_linearize(gp_vgicp_batch_t* b, const double* poses_host, gp_linearized6* out_dev) {
  if (!b || !poses_host || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_linearize: null");
  GP_TRY(ensure_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  GP_TRY(gp::stage_poses(b, poses_host, nullptr, &ps));
  return gp::launch_linearize(b, ps, out_dev, takes_rigid_path(b, poses_host));
}

// which kernels the host-pose entry points run at these poses: 1 = the 29 sums + adjoint expansion (every 3x3 block orthonormal to 1e-9, no pose far from its
// source cloud: takes_rigid_path), 0 = the explicit-J_s sums.  What a caller of gp_vgicp_batch_issue_linearize_dev passes as `rigid` to choose the same.
int gp_vgicp_batch_takes_rigid_path(gp_vgicp_batch_t* b, const double* poses_host, int* out) {
  if (!b || !poses_host || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_takes_rigid_path: null");
  GP_TRY(ensure_table(b));
  *out = takes_rigid_path(b, poses_host) ? 1 : 0;
  return GP_OK;
}

int gp_vgicp_factor_takes_rigid_path(gp_vgicp_factor_t* f, const double pose[16], int* out) {
  if (!f || !pose || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_factor_takes_rigid_path: null");
  GP_TRY(ensure_self_batch(f));
  *out = takes_rigid_path(f->self_batch, pose) ? 1 : 0;
  return GP_OK;
}

int gp_vgicp_batch_issue_compute_error(gp_vgicp_batch_t* b, const double* poses_lin_host, const double* poses_eval_host, double* out_dev) {
  if (!b || !poses_lin_host || !poses_eval_host || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_compute_error: null");
  GP_TRY(ensure_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps;
  GP_TRY(gp::stage_poses(b, poses_lin_host, poses_eval_host, &ps));
  return launch_error(b, ps, out_dev);
}

// the same two passes with the poses ALREADY in device memory (double[F][16] per table, column-major -- what a device-side retract produces, gp_lm.hip): no staging,
// no H2D copy, nothing for the host to wait on before the next call.  rigid: the caller vouches that every 3x3 block is orthonormal to 1e-9 (what the host-pose entry
// points test for themselves, poses_are_rigid): the 29-sum kernel + adjoint expansion; 0 = the 92-sum kernel, exact for any 3x3 block.  Any F (a single factor reads its descriptor and pose from the
// tables like the batch's other members: the in-argument form needs the pose on the host).
int gp_vgicp_batch_issue_linearize_dev(gp_vgicp_batch_t* b, const double* poses_dev, int rigid, gp_linearized6* out_dev) {
  if (!b || !poses_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_linearize_dev: null");
  GP_TRY(ensure_table(b));
  if (b->factors.empty()) return GP_OK;
  // (the by-factor fused finalize of the synchronous call was tried here too -- records written by the factors' last tile workgroups, no finalize launch -- and measured
  //  4 us SLOWER on BASELINE configs[2]'s batch: 59 us against 49.6 + 5.0, the 256 factors' tails end later than one finalize kernel over all of them; the error
  //  evaluation below keeps its fused form: 52 us against 49.5 + 9.2)
  return gp::launch_linearize(b, gp::device_poses(poses_dev), out_dev, rigid != 0);
}

int gp_vgicp_batch_issue_compute_error_dev(gp_vgicp_batch_t* b, const double* poses_lin_dev, const double* poses_eval_dev, double* out_dev) {
  if (!b || !poses_lin_dev || !poses_eval_dev || !out_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_compute_error_dev: null");
  GP_TRY(ensure_table(b));
  if (b->factors.empty()) return GP_OK;
  return launch_error(b, gp::device_poses(poses_lin_dev, poses_eval_dev), out_dev);
}

// ... and the error evaluation as a SYNCHRONOUS call: the finalize kernel hands the F sums and a completion word each to the host (pinned), and the call polls the words
// (wait_done) instead of going through hipStreamSynchronize -- everything queued in front of it on the batch's stream is complete when it returns, whatever else was
// queued BEHIND it in the meantime is not waited for (gp_lm.hip queues the next linearise there)
int gp_vgicp_batch_compute_error_dev(gp_vgicp_batch_t* b, const double* poses_lin_dev, const double* poses_eval_dev, double* out_host) {
  if (!b || !poses_lin_dev || !poses_eval_dev || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_compute_error_dev: null");
  GP_TRY(gp_vgicp_batch_issue_compute_error_dev_begin(b, poses_lin_dev, poses_eval_dev));
  return gp_vgicp_batch_compute_error_dev_end(b, out_host);
}

// the two halves of the call above: begin launches (and returns the moment the kernels are queued), end polls and copies.  One begin at a time per batch.
int gp_vgicp_batch_issue_compute_error_dev_begin(gp_vgicp_batch_t* b, const double* poses_lin_dev, const double* poses_eval_dev) {
  if (!b || !poses_lin_dev || !poses_eval_dev) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_issue_compute_error_dev_begin: null");
  GP_TRY(ensure_table(b));
  if (b->factors.empty()) return GP_OK;
  PoseSource ps = gp::device_poses(poses_lin_dev, poses_eval_dev);
  const gp::DoneFlags done = gp::next_done(b);
  b->arrival.dev_error_fused = false;
  if (b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !b->trace && !b->planned) {
    // ONE launch, as the synchronous call's by-factor form (gp_vgicp_batch_compute_error): the factor's last tile workgroup adds its rows up and hands sum and word over
    double* partials = nullptr;
    GP_TRY(gp::launch_fused_factors<gp::MODE_ERR>(b, &ps, nullptr, done, &partials));
    b->arrival.dev_error_fused = true;
    b->arrival.dev_error_lin = poses_lin_dev, b->arrival.dev_error_eval = poses_eval_dev;
    return GP_OK;
  }
  return launch_error(b, ps, static_cast<double*>(b->h_out_dev), done);
}

int gp_vgicp_batch_compute_error_dev_end(gp_vgicp_batch_t* b, double* out_host) {
  if (!b || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_compute_error_dev_end: null");
  const size_t F = b->factors.size();
  if (F == 0) return GP_OK;
  gp_vgicp_arrival& a = b->arrival;
  if (a.dev_error_fused) {
    // (as gp_vgicp_batch_compute_error: a counter left dirty by a launch that did not run to its end.)  Unlike the synchronous call, the rows of the pass cannot be
    // summed again here: work queued behind _begin on the batch's stream -- gp_lm.hip's speculative linearise -- writes the same partials buffer.  So the pass runs
    // again in its two-kernel form (tile kernel + vgicp_finalize_error_kernel, the order of sums the fused form keeps) at the poses _begin was given, behind
    // everything queued so far.
    GP_TRY(finish_fused(
        b, Arrival::by_factor, F, a.seq, true,
        [&](const gp::DoneFlags& again) { return launch_error(b, gp::device_poses(a.dev_error_lin, a.dev_error_eval), static_cast<double*>(b->h_out_dev), again); }, nullptr, true));
    a.dev_error_fused = false;
  } else {
    GP_TRY(gp::wait_words(b, F, a.seq, 400));  // (+ the damped step queued in front of it)
  }
  memcpy(out_host, b->h_out.ptr, sizeof(double) * F);
  return GP_OK;
}

int gp_vgicp_batch_stream(const gp_vgicp_batch_t* b, gp_stream_t* out) {
  if (!b || !out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_stream: null");
  *out = (gp_stream_t)b->stream;
  return GP_OK;
}

int gp_vgicp_batch_sync(gp_vgicp_batch_t* b) {
  if (!b) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "null batch");
  GP_HIP(hipStreamSynchronize(b->stream));
  return GP_OK;
}

int gp_vgicp_batch_linearize(gp_vgicp_batch_t* b, const double* poses_host, gp_linearized6* out_host) {
  if (!b || !poses_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_linearize: null");
  return batch_linearize_sync(b, poses_host, out_host, nullptr);
}

int gp_vgicp_batch_linearize_view(gp_vgicp_batch_t* b, const double* poses_host, const gp_linearized6** out_view) {
  if (!b || !poses_host || !out_view) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_linearize_view: null");
  return batch_linearize_sync(b, poses_host, nullptr, out_view);
}

int gp_vgicp_batch_compute_error(gp_vgicp_batch_t* b, const double* poses_lin_host, const double* poses_eval_host, double* out_host) {
  if (!b || !poses_lin_host || !poses_eval_host || !out_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_vgicp_batch_compute_error: null");
  const size_t F = b->factors.size();
  if (F == 0) return GP_OK;
  GP_TRY(ensure_table(b));
  PoseSource ps;
  GP_TRY(gp::stage_poses(b, poses_lin_host, poses_eval_host, &ps, true));
  const gp::DoneFlags done = gp::next_done(b);
  double* const sums = static_cast<double*>(b->h_out_dev);
  double* partials = nullptr;
  const int parts = (F == 1 && ps.inl.use && b->family == GP_KERNEL_STREAM && b->num_tiles >= gp::kFinalizeSplitTiles) ? gp::kFinalizeParts : 1;
  if (parts > 1) {
    // one large factor: eight part sums, added here in slot order -- by the part's last tile workgroup (fused, one launch) or by a second kernel, which announces
    // itself with this call's words when fusing is off and with the recovered ones when the fused launch's words are missing (see batch_linearize_sync)
    auto second = [&](const gp::DoneFlags& d) {
      return gp::launch_finalize_error_parts(b->stream, partials, b->num_tiles, gp::rows_per_part(b, parts), parts, sums, (int)kRecordDoubles, d);
    };
    if (b->tuning.fused_finalize) {
      GP_TRY(gp::launch_fused_parts<gp::MODE_ERR>(b, &ps, parts, done, &partials));
      GP_TRY(finish_fused(b, Arrival::by_part, (size_t)parts, done.seq, true, second));
    } else {
      GP_TRY(gp::partials_ptr(b, &partials));
      GP_TRY(gp::launch_tiles<gp::MODE_ERR>(b, ps, partials));
      GP_TRY(second(done));
      GP_TRY(gp::wait_words(b, (size_t)parts, done.seq));
    }
    const double* p = static_cast<const double*>(b->h_out.ptr);
    double a = p[0];
    for (int q = 1; q < parts; q++) a += p[(size_t)q * kRecordDoubles];
    out_host[0] = a;
    return GP_OK;
  }
  if (b->family == GP_KERNEL_STREAM && b->tuning.fused_finalize && !b->trace) {
    // ONE launch (round 4): the workgroup that stores a factor's last row adds the factor's rows up -- in the order of vgicp_finalize_error_kernel -- and hands the sum and
    // the completion word to the host (the by-factor form of the linearise, gp_vgicp_stream.hpp); small single factors and batches alike.  If a word is missing, the
    // finalize kernel does this call's sums
    GP_TRY(gp::launch_fused_factors<gp::MODE_ERR>(b, &ps, nullptr, done, &partials));
    GP_TRY(finish_fused(b, Arrival::by_factor, F, done.seq, true, [&](const gp::DoneFlags& again) {
      return gp::launch_finalize_error_table(b->stream, b->d_factors.as<gp::FactorDesc>(), (int)F, partials, sums, again);
    }));
  } else {
    GP_TRY(launch_error(b, ps, sums, done));
    GP_TRY(gp::wait_words(b, F, done.seq));
  }
  memcpy(out_host, b->h_out.ptr, sizeof(double) * F);
  return GP_OK;
}

}  // extern "C"
