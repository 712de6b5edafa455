// gp_lm.hip -- one Levenberg-Marquardt trial over a graph of pairwise factors WITHOUT the host in the middle (round 6).
//
// The reference's optimizer drives its GPU factors from the host (optimizers/levenberg_marquardt_ext.cpp): iterate() :352-392 hands `values` to
// linearization_hook_->linearize (cuda/nonlinear_factor_set_gpu.cpp:64-101: poses up, kernels, records down), tryLambda() :188-350 builds the damped system, solves,
// retracts ON THE HOST (:239), hands the new values to linearization_hook_->error (:245, nonlinear_factor_set_gpu.cpp:103-139: poses up, kernels, errors down) and
// decides.  Two waits, two uploads and the pose algebra of every factor per trial -- fine beside a 1.5 s CPU linearise, 0.13 ms of a 0.39 ms iteration here
// (BASELINE configs[2]: 256 factors over 64 poses).
//
// Here the VALUES live in device memory beside the records:
//   gp_lm_graph_linearize    every group's linearise at the relative poses of the current values (a device table: PairGroup::issue_linearize) -> records in HBM
//   gp_lm_graph_try_lambda   the damped step (gp::DampedSystem::issue_step: the dense system for one free pose, else the block-sparse one), then the retract of the
//                            current values by the step's x (Pose3::retract = T Expmap(xi), (omega, v) order), which writes the trial values and every factor's relative
//                            pose -- as the EPILOGUE of the step's own kernel where the step is one launch (gp_lm_poses.hpp), else one small kernel behind it
//                            (lm_poses_kernel) --, then every group's error evaluation on the linearisation's correspondences at those (PairGroup::error_begin / _end):
//                            launches queued back to back, ONE wait -- a poll of the error evaluation's completion words, not hipStreamSynchronize -- with the
//                            linearise at the trial values already queued behind them (speculation: an accepted step finds it running); x, b, c, the trial's
//                            error and the trial values reach the host through pinned memory
//   gp_lm_graph_accept       the trial values become the current ones (their relative poses are already in place for the next linearise): a pointer swap
//   gp_lm_graph_optimize     the reference's cadence over those three (tryLambda's tests :262-292, decreaseLambda / increaseLambda with the GTSAM defaults)
// Pose arithmetic on the device = the formulas of gtsam::Pose3 (Expmap with the closed-form V, compose, inverse() * other) in f64; the host-side harness
// (bench_lm.py) computes the same with numpy, and the two agree to rounding (tests/test_lm_gpu.py).
// The pairwise factors are a TABLE of groups (gp_lm_groups.hpp: the VGICP batch, then the GICP / ICP batch of gp_corr_batch.hip), each with its pairs, its two delta
// tables (written by the same retract), its errors and its run of the records; the pose factors' records follow the last group's.  A new factor family is one more row
// of that table and its three operations.  The correspondence batch keeps its correspondences in two SETS -- set `rec` goes with record buffer `rec`, the
// speculative linearise at a trial's values searches into set 1 - rec, so a rejected trial leaves the correspondences of the linearisation point where the next
// trial's error evaluation reads them.
// Device: the graph is created on the device that is current (the batch's: gp_set_device first in a multi-device process), like the batch and the systems it builds.
// Not thread-safe per handle, re-entrant across handles, like the rest of the library.
#include <cmath>
#include <cstring>
#include <limits>
#include <memory>
#include <vector>

#include "gp_host.hpp"
#include "gp_lm_groups.hpp"
#include "gp_lm_poses.hpp"
#include "gp_pose_factors.hpp"
#include "gp_vgicp_shared.hpp"

namespace gp {

__global__ void __launch_bounds__(256) lm_poses_kernel(const LmPoseView v) {
  lm_poses_thread(v, blockIdx.x * 256 + threadIdx.x, v.x, v.x != nullptr && *v.status != 0);
}

// One group of pairwise factors: a batch (not owned; neither = the graph has no factor of this family, count = 0) and what the graph keeps per factor of it.  The
// three operations are the batches' own entry points under one shape.
struct PairGroup {
  gp_vgicp_batch_t* vgicp = nullptr;  // group kLmVgicp
  gp_corr_batch_t* corr = nullptr;    // group kLmCorr: correspondence set k goes with d_records[k]
  int count = 0, record_offset = 0;   // records [record_offset, record_offset + count) of both record buffers
  std::vector<int> pairs;             // host copy of (target pose, source pose), for the far-pose rule at set_values
  gp::DeviceArray d_pairs, d_deltas[2];
  std::vector<double> errors;
  bool active() const { return vgicp || corr; }
  // the linearise at `deltas` into this group's run of `records` (the VGICP batch has no correspondence sets: it ignores `set`)
  int issue_linearize(const double* deltas, bool rigid, int set, gp_linearized6* records) {
    return vgicp ? gp_vgicp_batch_issue_linearize_dev(vgicp, deltas, rigid ? 1 : 0, records + record_offset)
                 : gp_corr_batch_issue_linearize_dev(corr, deltas, rigid ? 1 : 0, set, records + record_offset);
  }
  // the errors at deltas_eval on the correspondences of the linearisation at deltas_lin (set rec_set), in two halves: queued, then awaited into `errors`
  int error_begin(int rec_set, const double* deltas_lin, const double* deltas_eval) {
    return vgicp ? gp_vgicp_batch_issue_compute_error_dev_begin(vgicp, deltas_lin, deltas_eval) : gp::corr_batch_error_begin(corr, rec_set, deltas_lin, deltas_eval);
  }
  int error_end(long extra_spin_us) { return vgicp ? gp_vgicp_batch_compute_error_dev_end(vgicp, errors.data()) : gp::corr_batch_error_end(corr, errors.data(), extra_spin_us); }
};

}  // namespace gp

struct gp_lm_graph {
  gp::PairGroup groups[gp::kLmGroups];
  std::unique_ptr<gp::DampedSystem> system;  // one free pose: the dense step (a 6 x 6 system); else the block-sparse one
  hipStream_t stream = nullptr;
  int N = 0, slots = 0;
  // pose factors (gp_pose_factors.hpp): records [pose_record_offset, + P) of both record buffers; their errors at a trial's values reach the host through h_pose_errors, written by
  // the launch that also writes their records at those values (speculation) -- queued in front of the batches' error evaluation, so its completion words cover them
  int P = 0, pose_record_offset = 0;
  gp::DeviceArray d_pose_factors;
  gp::PinnedArray h_pose_errors;
  gp::DeviceArray d_slot, d_values[2], d_records[2];
  gp::PinnedArray h_values[2];
  int cur = 0;                 // d_values[cur] / d_deltas[cur] / h_values[cur] are the current values; [1 - cur] the last trial's
  bool have_values = false, linearized = false, tried = false;
  bool rigid = true;           // every value handed to set_values was orthonormal to 1e-9 (retracts keep them so): the rigid kernels, as the host-pose entry points would choose
  // speculation: behind a trial's error evaluation the linearise AT THE TRIAL VALUES is queued into the other record buffer, so that an accepted step -- the common
  // case -- finds its linearisation already running while the host still decides; a rejected one leaves the records of the linearisation point untouched for the next
  // lambda (the queued linearise is 50 us of device time thrown away).  Same kernels on the same operands either way: results do not depend on it.
  int rec = 0;                 // d_records[rec]: the records of the current linearisation point
  bool speculate = true, spec_pending = false /* [1 - rec] is being written at the last trial's values */, spec_valid = false /* [rec] already holds the current values' records */;
  const double* x_dev = nullptr;
  const int* status_dev = nullptr;
  ~gp_lm_graph() {
    if (system) (void)hipStreamSynchronize(stream);  // (in front of the members' release: the system's buffers and the tables may still be in use)
  }
  gp_linearized6* records(int k) { return d_records[k].as<gp_linearized6>(); }
};

namespace {

gp::LmPoseView pose_view(gp_lm_graph* g, int from, int to, bool step) {
  gp::LmPoseView v{};
  v.values = g->d_values[from].as<double>();
  v.slot = g->d_slot.as<int>();
  v.x = step ? g->x_dev : nullptr;
  v.status = g->status_dev;
  v.values_out = step ? g->d_values[to].as<double>() : nullptr;
  v.values_host = step ? g->h_values[to].as<double>() : nullptr;
  // (the view names the two groups one by one: with a table of groups in the view -- walked by a loop or by one helper call per group -- lm_poses_thread compiles to
  //  other fused multiply-adds in the VGICP group's between_rigid, and the relative poses change in their last bit.  Open work: DESIGN.md)
  const gp::PairGroup &vg = g->groups[gp::kLmVgicp], &cg = g->groups[gp::kLmCorr];
  v.pairs = vg.d_pairs.as<int>(), v.deltas_out = vg.d_deltas[to].as<double>(), v.F = vg.count, v.N = g->N;
  v.corr_pairs = cg.d_pairs.as<int>(), v.corr_deltas_out = cg.d_deltas[to].as<double>(), v.G = cg.count;
  return v;
}

int launch_poses(gp_lm_graph* g, int from, int to, bool step) {
  const gp::LmPoseView v = pose_view(g, from, to, step);
  const int n = v.threads();
  hipLaunchKernelGGL(gp::lm_poses_kernel, dim3((n + 255) / 256), dim3(256), 0, g->stream, v);
  GP_HIP(hipGetLastError());
  return GP_OK;
}

// The one create path.  `api` names the entry point in the messages; needs_batch: gp_lm_graph_create's own rule (a VGICP batch of >= 1 factors, >= 2 poses).  Every
// refusal is made on the host before any device work, in this order: the arguments, the pose factors, a graph without factors, the pairs group by group, all poses
// held, the streams.
int create_graph(const char* api, bool needs_batch, gp_vgicp_batch_t* batch, const int* pose_pairs, gp_corr_batch_t* corr, const int* corr_pairs,
                 const gp_pose_factor* pose_factors, int P, int num_poses, const unsigned char* pose_fixed, int ordering, gp_stream_t stream, gp_lm_graph_t** out) {
  const std::string a = std::string(api) + ": ";
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "null out");
  *out = nullptr;
  const int F = batch ? gp_vgicp_batch_size(batch) : 0, G = corr ? gp_corr_batch_size(corr) : 0;
  if (needs_batch && (!batch || F <= 0 || !pose_pairs || num_poses < 2)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "a batch of >= 1 factors, pose_pairs [F][2], >= 2 poses");
  if (F < 0 || (F > 0 && !pose_pairs)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "pose_pairs [F][2]");
  if (corr && (G <= 0 || !corr_pairs || num_poses < 2)) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "corr_pairs [G][2], >= 2 poses");
  GP_TRY(gp::check_pose_factors(pose_factors, P, num_poses, api));
  if (F + G + P == 0) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "a graph without factors");
  const int* const pairs[gp::kLmGroups] = {pose_pairs, corr_pairs};
  const int count[gp::kLmGroups] = {F, G};
  gp::LmLayout L;
  const std::string refusal = gp::lm_layout(pairs, count, pose_factors, P, num_poses, pose_fixed, &L);
  if (!refusal.empty()) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + refusal);
  gp_stream_t st = stream;
  if (batch) GP_TRY(gp_vgicp_batch_stream(batch, &st));
  if (batch && stream && stream != st) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "stream must be NULL or the batch's own");
  if (corr) {
    gp_stream_t cs = nullptr;
    GP_TRY(gp_corr_batch_stream(corr, &cs));
    if (batch && cs != st) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "the two batches must share one stream");
    if (!batch && stream && stream != cs) return gp::fail(GP_ERROR_INVALID_ARGUMENT, a + "stream must be NULL or the batches' own");
    if (!batch) st = cs;
  }
  auto g = std::make_unique<gp_lm_graph>();
  g->groups[gp::kLmVgicp].vgicp = batch, g->groups[gp::kLmCorr].corr = corr;
  g->N = num_poses, g->slots = L.slots, g->P = P, g->pose_record_offset = L.record_offset[gp::kLmGroups];
  g->stream = (hipStream_t)st;
  if (L.slots == 1) {
    gp_dense_system_t* dense = nullptr;
    GP_TRY(gp_dense_system_create(1, L.factor_slots.data(), L.num_records, st, &dense));
    g->system.reset(gp::as_damped_system(dense));
  } else {
    gp_sparse_system_t* sparse = nullptr;
    GP_TRY(gp_sparse_system_create(L.slots, L.factor_slots.data(), L.num_records, ordering, st, &sparse));
    g->system.reset(gp::as_damped_system(sparse));
  }
  g->system->device_solution(&g->x_dev, &g->status_dev);
  for (int k = 0; k < gp::kLmGroups; k++) {
    gp::PairGroup& p = g->groups[k];
    p.count = count[k], p.record_offset = L.record_offset[k];
    if (count[k] > 0) p.pairs.assign(pairs[k], pairs[k] + 2 * (size_t)count[k]);
    p.errors.assign((size_t)count[k], 0.0);
    GP_TRY(gp::upload(p.d_pairs, p.pairs));
    for (int j = 0; j < 2; j++) GP_TRY(p.d_deltas[j].alloc(sizeof(double) * 16 * (size_t)count[k]));
  }
  const size_t vb = sizeof(double) * 16 * (size_t)num_poses;
  for (int j = 0; j < 2; j++) {
    GP_TRY(g->d_values[j].alloc(vb));
    GP_TRY(g->h_values[j].ensure(vb));
    GP_TRY(g->d_records[j].alloc(sizeof(gp_linearized6) * (size_t)L.num_records));
  }
  GP_TRY(gp::upload(g->d_slot, L.slot));
  if (P > 0) {
    GP_TRY(g->d_pose_factors.alloc(sizeof(gp_pose_factor) * (size_t)P));
    GP_TRY(g->h_pose_errors.ensure(sizeof(double) * (size_t)P));
    GP_HIP(hipMemcpy(g->d_pose_factors.ptr, pose_factors, sizeof(gp_pose_factor) * (size_t)P, hipMemcpyHostToDevice));
  }
  *out = g.release();
  return GP_OK;
}

}  // namespace

extern "C" {

int gp_lm_graph_destroy(gp_lm_graph_t* g) {
  delete g;
  return GP_OK;
}

int gp_lm_graph_create(gp_vgicp_batch_t* batch, const int* pose_pairs, int num_poses, const unsigned char* pose_fixed, int ordering, gp_lm_graph_t** out) {
  return create_graph("gp_lm_graph_create", true, batch, pose_pairs, nullptr, nullptr, nullptr, 0, num_poses, pose_fixed, ordering, nullptr, out);
}

int gp_lm_graph_create_with_pose_factors(gp_vgicp_batch_t* batch, const int* pose_pairs, const gp_pose_factor* pose_factors, int num_pose_factors, int num_poses,
                                         const unsigned char* pose_fixed, int ordering, gp_stream_t stream, gp_lm_graph_t** out) {
  return create_graph("gp_lm_graph_create_with_pose_factors", false, batch, pose_pairs, nullptr, nullptr, pose_factors, num_pose_factors, num_poses, pose_fixed, ordering, stream, out);
}

// (without a correspondence batch this IS gp_lm_graph_create_with_pose_factors, and says so in its refusals)
int gp_lm_graph_create_with_factors(gp_vgicp_batch_t* batch, const int* vgicp_pairs, gp_corr_batch_t* corr, const int* corr_pairs, const gp_pose_factor* pose_factors,
                                    int num_pose_factors, int num_poses, const unsigned char* pose_fixed, int ordering, gp_stream_t stream, gp_lm_graph_t** out) {
  if (!out) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_create_with_factors: null out");
  return create_graph(corr ? "gp_lm_graph_create_with_factors" : "gp_lm_graph_create_with_pose_factors", false, batch, vgicp_pairs, corr, corr_pairs, pose_factors, num_pose_factors,
                      num_poses, pose_fixed, ordering, stream, out);
}

// 0: no linearise is queued ahead of the host's decision (measurement / A-B; results are the same bits either way).  Returns the previous setting.
int gp_lm_graph_set_speculation(gp_lm_graph_t* g, int enable) {
  if (!g) return 0;
  const int was = g->speculate ? 1 : 0;
  g->speculate = enable != 0;
  return was;
}

// the graph's own damped system: 0 = its multi-launch step (the retract then runs as lm_poses_kernel behind it), 1 = the one-launch step where the system qualifies
// (default; the retract is its epilogue).  Bit-identical; for the test that says so and A/B timing.  Returns what the next trial runs (as gp_*_system_set_one_launch).
int gp_lm_graph_set_one_launch(gp_lm_graph_t* g, int enable) { return g ? g->system->set_one_launch(enable) : 0; }

int gp_lm_graph_num_variables(const gp_lm_graph_t* g) { return g ? 6 * g->slots : 0; }

int gp_lm_graph_set_values(gp_lm_graph_t* g, const double* values_host) {
  if (!g || !values_host) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_set_values: null");
  bool rigid = true;
  for (int i = 0; i < g->N; i++) rigid = rigid && gp::pose_is_rigid(values_host + 16 * (size_t)i);
  if (g->P > 0 && !rigid) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_set_values: a graph with pose factors takes rigid values (orthonormal to 1e-9, det > 0)");
  GP_HIP(hipStreamSynchronize(g->stream));  // (a trial in flight still writes the pinned values)
  const gp::PairGroup& vg = g->groups[gp::kLmVgicp];
  if (rigid && vg.vgicp && vg.count > 0) {
    // ... and no VGICP factor's relative pose inverse(T_t) T_s is far from its source cloud (gp_vgicp_batch_takes_rigid_path: the rule of the host-pose entry points, decided
    // here for the values as set; the retracts that follow move them by steps, not by kilometres).  Only |t| of the relative pose enters the rule, and
    // |Ra^T (tb - ta)| = |tb - ta|: the rotation blocks asked about are identities, so that rounding in a product of two rotations cannot change the answer above
    std::vector<double> rel(16 * (size_t)vg.count, 0.0);
    for (int f = 0; f < vg.count; f++) {
      const double* A = values_host + 16 * (size_t)vg.pairs[2 * (size_t)f];
      const double* B = values_host + 16 * (size_t)vg.pairs[2 * (size_t)f + 1];
      double* D = rel.data() + 16 * (size_t)f;  // column-major
      D[0] = D[5] = D[10] = D[15] = 1.0;
      for (int r = 0; r < 3; r++) D[12 + r] = B[12 + r] - A[12 + r];
    }
    int near = 1;
    GP_TRY(gp_vgicp_batch_takes_rigid_path(vg.vgicp, rel.data(), &near));
    rigid = near != 0;
  }
  g->rigid = rigid;
  memcpy(g->h_values[g->cur].ptr, values_host, sizeof(double) * 16 * (size_t)g->N);
  GP_HIP(hipMemcpyAsync(g->d_values[g->cur].ptr, g->h_values[g->cur].ptr, sizeof(double) * 16 * (size_t)g->N, hipMemcpyHostToDevice, g->stream));
  GP_TRY(launch_poses(g, g->cur, g->cur, false));
  g->have_values = true, g->linearized = false, g->tried = false, g->spec_pending = false, g->spec_valid = false;
  return GP_OK;
}

int gp_lm_graph_get_values(gp_lm_graph_t* g, double* values_host) {
  if (!g || !values_host || !g->have_values) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_get_values: no values");
  memcpy(values_host, g->h_values[g->cur].ptr, sizeof(double) * 16 * (size_t)g->N);
  return GP_OK;
}

int gp_lm_graph_linearize(gp_lm_graph_t* g) {
  if (!g || !g->have_values) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_linearize: set the values first");
  if (!g->spec_valid) {  // (else: queued behind the accepted trial's error evaluation)
    for (gp::PairGroup& p : g->groups)
      if (p.active()) GP_TRY(p.issue_linearize(p.d_deltas[g->cur].as<double>(), g->rigid, g->rec, g->records(g->rec)));
    GP_TRY(gp::launch_pose_factors(g->d_pose_factors.as<gp_pose_factor>(), g->P, g->d_values[g->cur].as<double>(), g->records(g->rec) + g->pose_record_offset, nullptr, g->stream));
  }
  g->spec_valid = false;
  g->linearized = true, g->tried = false;
  return GP_OK;
}

int gp_lm_graph_records(gp_lm_graph_t* g, const gp_linearized6** records_dev, const double** relative_poses_dev) {
  if (!g) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_records: null graph");
  if (records_dev) *records_dev = g->records(g->rec);
  if (relative_poses_dev) *relative_poses_dev = g->groups[gp::kLmVgicp].d_deltas[g->cur].as<double>();
  return GP_OK;
}

// The order on the stream, which every loop below keeps: (1) the damped step, (2) the retract -- the step's epilogue or lm_poses_kernel --, (3) the pose factors,
// (4) the groups' error_begin LAST GROUP FIRST (the correspondence batch's, then the VGICP batch's), (5) the speculative linearises in group order (VGICP, then
// correspondence), (6) the groups' error_end in group order, (7) the step's collect / finish.
int gp_lm_graph_try_lambda(gp_lm_graph_t* g, double lambda, int diagonal_damping, double min_diagonal, double max_diagonal, double* x_host, double* b_host, double* c_host,
                           double* new_error, double* new_values_host) {
  if (!g || !g->linearized) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_try_lambda: linearize first");
  const int to = 1 - g->cur;
  g->spec_pending = false, g->tried = false;
  // (the one-launch steps retract the poses themselves, as their epilogue: gp_lm_poses.hpp; behind a multi-launch step lm_poses_kernel does)
  bool fused = false;
  const gp::LmPoseView pv = pose_view(g, g->cur, to, true);
  GP_TRY(g->system->issue_step(g->records(g->rec), gp::Damping{lambda, diagonal_damping, min_diagonal, max_diagonal}, nullptr, &pv, &fused));
  int rc = fused ? GP_OK : launch_poses(g, g->cur, to, true);
  // the pose factors at the trial values the retract has just written (an indeterminate step leaves them = the current values): their errors, and with speculation
  // their records for the next linearisation, in one launch -- in front of the batches' error evaluation, whose completion words therefore cover them
  if (rc == GP_OK)
    rc = gp::launch_pose_factors(g->d_pose_factors.as<gp_pose_factor>(), g->P, g->d_values[to].as<double>(), g->speculate ? g->records(1 - g->rec) + g->pose_record_offset : nullptr,
                                 g->h_pose_errors.as<double>(), g->stream);
  // every group's errors at the trial deltas, on the correspondences of the linearisation point (set rec)
  bool any_batch = false;
  for (int k = gp::kLmGroups - 1; k >= 0; k--) {
    gp::PairGroup& p = g->groups[k];
    any_batch = any_batch || p.active();
    if (rc == GP_OK && p.active()) rc = p.error_begin(g->rec, p.d_deltas[g->cur].as<double>(), p.d_deltas[to].as<double>());
  }
  if (rc != GP_OK) {  // the step went out: collect it (its own wait) before the error is reported
    (void)g->system->finish(true, nullptr, nullptr, nullptr);
    return rc;
  }
  // (the correspondence batch into its OTHER set: a rejected trial must leave set rec as the linearisation point's.  A speculative launch that fails is swallowed on
  //  purpose: spec = false, and the next gp_lm_graph_linearize issues the linearise itself and reports its error)
  bool spec = g->speculate;
  for (gp::PairGroup& p : g->groups)
    if (spec && p.active()) spec = p.issue_linearize(p.d_deltas[to].as<double>(), g->rigid, 1 - g->rec, g->records(1 - g->rec)) == GP_OK;
  // the call's ONE wait: the completion words of the error evaluation (everything in front of it on the stream -- the step, the trial values, the pose factors -- is
  // then complete and its pinned results are readable; the speculative linearise behind it is not waited for).  With both batches the VGICP words are behind the
  // correspondence batch's on the stream, so those have arrived and their poll returns at once.  Without a batch, or after a failed poll: the step's own wait, behind
  // the pose factors' launch.
  constexpr long kStepSpinUs = 400;  // (+ the damped step queued in front of it)
  for (gp::PairGroup& p : g->groups)
    if (rc == GP_OK && p.active()) rc = p.error_end(kStepSpinUs);
  const int rs = g->system->finish(rc != GP_OK || !any_batch, x_host, b_host, c_host);
  if (rc != GP_OK) return rc;
  if (rs != GP_OK) return rs;  // GP_ERROR_INDETERMINATE: b, c valid; no trial (the kernel behind the step left the trial values = the current ones)
  g->tried = true;
  g->spec_pending = spec;
  if (new_error) {
    double e = 0.0;
    for (const gp::PairGroup& p : g->groups)
      for (const double v : p.errors) e += v;
    const double* pe = g->h_pose_errors.as<double>();
    for (int p = 0; p < g->P; p++) e += pe[p];
    *new_error = e;
  }
  if (new_values_host) memcpy(new_values_host, g->h_values[to].ptr, sizeof(double) * 16 * (size_t)g->N);
  return GP_OK;
}

int gp_lm_graph_accept(gp_lm_graph_t* g) {
  if (!g || !g->tried) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_accept: no successful trial to accept");
  g->cur = 1 - g->cur;
  if (g->spec_pending) g->rec = 1 - g->rec, g->spec_valid = true;
  g->spec_pending = false;
  g->tried = false, g->linearized = false;
  return GP_OK;
}

int gp_lm_graph_optimize(gp_lm_graph_t* g, const gp_lm_params* params, gp_lm_summary* summary) {
  if (!g || !g->have_values || !summary) return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_optimize: set the values first; summary must not be null");
  gp_lm_params p;
  gp_lm_params_default(&p);
  if (params) p = *params;
  if (!(p.lambda_initial > 0.0) || !(p.lambda_factor > 1.0) || p.max_iterations < 0 || p.diagonal_damping)
    return gp::fail(GP_ERROR_INVALID_ARGUMENT, "gp_lm_graph_optimize: lambda_initial > 0, lambda_factor > 1, lambda I damping only (drive gp_lm_graph_try_lambda yourself for the diagonal form)");
  const size_t n = 6 * (size_t)g->slots;
  std::vector<double> x(n), b(n);
  double lam = p.lambda_initial, err = std::numeric_limits<double>::quiet_NaN();
  *summary = gp_lm_summary{};
  bool stop = false;
  for (int it = 0; it < p.max_iterations && !stop; it++) {
    summary->iterations++;
    GP_TRY(gp_lm_graph_linearize(g));
    for (;;) {  // tryLambda until a step is taken or the search ends (levenberg_marquardt_ext.cpp:188-350)
      summary->inner_iterations++;
      double c = 0.0, new_err = 0.0;
      const int rc = gp_lm_graph_try_lambda(g, lam, p.diagonal_damping, p.min_diagonal, p.max_diagonal, x.data(), b.data(), &c, &new_err, nullptr);
      if (rc != GP_OK && rc != GP_ERROR_INDETERMINATE) return rc;
      err = c;  // the cost at the linearisation point comes back with the step, solved or not (the GPU factor keeps the linearise's error)
      bool accepted = false;
      if (rc == GP_OK) {
        double bx = 0.0, xx = 0.0;
        for (size_t i = 0; i < n; i++) bx += b[i] * x[i], xx += x[i] * x[i];
        const double lin_change = 0.5 * bx + 0.5 * lam * xx;  // old - new linearised error of (A + lambda I) dx = b  (:226-230)
        if (lin_change >= 0.0) {
          const double change = err - new_err;
          accepted = lin_change > std::numeric_limits<double>::epsilon() * err && change / lin_change > p.min_model_fidelity;  // (:262-268)
          if (std::fabs(change) < p.relative_error_tol * err) stop = true;                                                     // (:271-278)
        }
        if (accepted) {
          const double prev = err;
          GP_TRY(gp_lm_graph_accept(g));
          err = new_err;
          lam /= p.lambda_factor;
          if (lam < p.lambda_lower_bound) lam = p.lambda_lower_bound;
          if (std::fabs(prev - err) < p.absolute_error_tol || std::fabs(prev - err) / std::max(prev, 1e-300) < p.relative_error_tol) stop = true;  // optimize() :394-430
          break;
        }
      }
      if (stop) break;
      lam *= p.lambda_factor;
      if (lam >= p.lambda_upper_bound) {
        stop = true;
        summary->gave_up = 1;
        break;
      }
    }
  }
  summary->final_error = err;
  summary->final_lambda = lam;
  return GP_OK;
}

void gp_lm_params_default(gp_lm_params* p) {
  if (!p) return;
  p->lambda_initial = 1e-5, p->lambda_factor = 10.0, p->lambda_upper_bound = 1e5, p->lambda_lower_bound = 0.0;
  p->relative_error_tol = 1e-5, p->absolute_error_tol = 1e-5, p->min_model_fidelity = 1e-3;
  p->min_diagonal = 1e-6, p->max_diagonal = 1e32;
  p->max_iterations = 100, p->diagonal_damping = 0;
}

}  // extern "C"
