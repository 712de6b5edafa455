// gp_vgicp_batch.hpp -- the VGICP factor and batch as every unit of the VGICP path sees them: gp_vgicp.hip (kernels and their launches), gp_vgicp_table.hip (tuning,
// factor / tile tables, pose staging), gp_vgicp_batch.hip (the entry points the product calls; the arrival protocol of the fused finalize is gp_vgicp_arrival.hpp)
// and gp_vgicp_debug.hip (check hooks and measurement).
#pragma once

#include <algorithm>
#include <cstring>
#include <memory>
#include <vector>

#include "gp_host.hpp"
#include "gp_vgicp_plan.hpp"

struct gp_vgicp_batch;

// Per-batch tuning (gp_vgicp_batch_set_tuning / gp_vgicp_factor_set_tuning; keys GP_TUNE_* of gtsam_points_hip.h).  Nothing here is process-global:
// two batches on two threads may run different kernels side by side (re-entrant across handles).
struct gp_vgicp_tuning {
  int kernel = GP_KERNEL_STREAM;  // GP_KERNEL_*: which tile kernel family the batch prefers (it falls back where that family does not apply)
  int source_policy = 0;          // cache policy of the source stream: 0 = per batch (non-temporal iff no two factors share a source cloud), 1 = default, 2 = non-temporal
  int xcd_chunk = 0;              // workgroup -> tile map: 0 = every XCD walks a contiguous eighth of the tile list, c > 0 = runs of c tiles dealt round robin
  int stagger = 0;                // round-2 kernels: odd wave slots start `stagger` x 512 clocks late
  int tile_interleave = 0;        // consecutive factors that share a source cloud take turns tile by tile
  int xcd_weights[8] = {1000, 1000, 1000, 1000, 1000, 1000, 1000, 1000};  // GP_TUNE_XCD_WEIGHT_0 + x: share of XCD x in 1/1000 of the mean (unset: the library's table)
  bool xcd_weights_set = false;
  int max_wgs = 1024;             // stream family, one large factor: workgroups of the planned launch (<= one resident round of 1024)
  int tile_chunks = 0;            // stream family, batches: 64-point chunks per wave of a tile (tile = 256 x this many points); 0 = the largest of 4 / 2 / 1 that fills 3/4 of the chip
  int fused_finalize = 1;         // synchronous rigid calls of the stream family, single factors and batches: the last tile workgroup of each part of a large factor,
                                  // or of each factor, sums the rows and hands them to the host (InlinePoses: fused finalize) -- no finalize launch.  (The first form
                                  // of this knob, finalize workgroups on a second stream waiting for the counters, cost +10 us per step: profiles/r03_overlap_finalize.jsonl)
  int balance = gp::kDefaultSkewPermille;  // stream kernel, one large factor: how much more a dispatch round takes than the next, in 1/1000 of the mean share (0 = flat)
  int source_mirror = 1;          // stream family: stream the sources' packed mirrors (36 B per point, gp::SourceMirror) when every factor of the batch has one; 0 = the caller's arrays
  int far_pose_ratio = GP_FAR_POSE_RATIO_DEFAULT;  // GP_TUNE_FAR_POSE_RATIO: a rigid pose with |t| > this x the source cloud's extent takes the explicit-J_s sums (0 = none does)
};

struct gp_vgicp_factor {
  const gp_voxelmap* target = nullptr;
  const float* points = nullptr;
  const float* covs = nullptr;
  const float* normals = nullptr;
  int n = 0;
  int device = 0;  // the device the source arrays live on (hipPointerGetAttributes at creation)
  bool surface_validation = false;
  uint64_t generation = 0;  // bumped when the source pointers or flags change (tables that hold this factor go stale)
  double extent = 0.0;      // largest |coordinate| of the source's finite points (source_extent_kernel, at the first table build that holds this factor) ...
  uint64_t extent_generation = ~0ull;  // ... for this generation of the source arrays
  double inlier_thresh_trans = 1e-6, inlier_thresh_angle = 1e-6;  // integrated_vgicp_derivatives.cu:26-27 (kept for API parity)
  hipStream_t stream = nullptr;
  bool owns_stream = false;
  gp_temp_buffer* temp_buffer = nullptr;
  bool owns_temp_buffer = false;
  std::shared_ptr<gp::SourceMirror> mirror;  // packed mirror of (points, covs, n), shared with the other factors on this cloud; acquired by the first table build that wants it
  bool mirror_tried = false;                 // ... which happened (a cloud of < 64 points has none)
  gp_vgicp_batch* self_batch = nullptr;  // lazily built batch of one, used by the per-factor entry points
  gp_vgicp_tuning tuning;                // what the self batch is created with (gp_vgicp_factor_set_tuning)
};

// the arrival state of the fused finalize (gp_vgicp_arrival.hpp): the counters the tile workgroups arrive at, what the host believes they read, and the completion
// words the host polls
struct gp_vgicp_arrival {
  gp::DeviceArray d_arrive;               // by part: 16 monotonic arrival counters, kArriveStride words apart
  unsigned long long arrived[16] = {0};   // ... what they read once every launch issued so far has finished
  gp::DeviceArray d_factor_arrive;        // by factor: one counter per factor, kFactorArriveStride words apart, zero between launches
  size_t factor_arrive_count = 0;
  bool factor_arrive_dirty = false;       // a by-factor fused launch went out and has not been seen to complete: the zero-reset counters may be anywhere
  gp::PinnedArray h_done;  // one completion word per factor, written by the finalize kernel behind its record (synchronous calls poll it)
  void* h_done_dev = nullptr;
  unsigned long long seq = 0;
  bool dev_error_fused = false;  // gp_vgicp_batch_issue_compute_error_dev_begin went out in the by-factor fused form
  const double* dev_error_lin = nullptr;   // ... at these device pose tables: what _end runs the pass again with when the completion words are missing
  const double* dev_error_eval = nullptr;
  int drop_error_words = 0;      // test hook (gp_debug_drop_error_words): the next so many fused error evaluations take the "words did not arrive" branch
};

// what a batch measures about itself (gp_vgicp_debug.hip reads it out).  The events and the trace buffer that the launches themselves touch are the batch's ev / trace.
struct gp_vgicp_measurement {
  bool timing = false;  // GP_TUNE_TIMING: the synchronous linearise brackets its two kernels with HIP events (gp_vgicp_batch_last_kernel_ms)
  float last_tile_ms = 0.f, last_finalize_ms = 0.f;
  // fused steps: the kernel's own 100 MHz time stamps (gp_vgicp_batch_device_times)
  double dev_steps = 0.0, dev_stream_ticks = 0.0, dev_kernel_ticks = 0.0;
};

struct gp_vgicp_batch {
  std::vector<gp_vgicp_factor*> factors;
  hipStream_t stream = nullptr;
  gp_temp_buffer* temp_buffer = nullptr;  // partials arena when provided (per-stream scratch), else own
  int num_tiles = 0;
  gp_vgicp_tuning tuning;
  int family = 0;         // GP_KERNEL_* the tile table was built for (tuning.kernel after the fallbacks)
  bool nt = false;        // source stream non-temporal (tuning.source_policy resolved)
  bool any_sv = false;    // some factor validates surfaces
  bool packed = false;    // every factor streams its packed mirror (vgicp_stream_kernel<PK>)
  bool planned = false;   // stream kernel, one large factor: the tile list is a balanced StreamPlan (else fixed tiles of tile_points)
  gp::StreamPlan plan{};  // ... how the chunks are dealt (also written into the tile table)
  unsigned long long* trace = nullptr;  // timeline build of the tile kernel: [2048][16] uint64 device buffer (gp_vgicp_batch_set_trace_buffer)
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};  // measurement.timing: around the two kernels of a timed linearise (launch_linearize records them)
  gp_vgicp_arrival arrival;          // fused finalize (GP_TUNE_FUSED_FINALIZE; synchronous rigid calls of the stream family)
  gp_vgicp_measurement measurement;
  int tile_points = 0;
  int64_t total_points = 0;
  gp::DeviceArray d_factors, d_tiles, d_partials, d_poses;  // d_poses: [2][F][16] (lin, eval)
  bool use_grid = false;  // every factor's map carries an occupancy-block grid (else the hashed line table is used)
  bool stream_once = false;  // no two factors of the batch read the same source cloud (and no sibling batch on this device does: gp_multi.hip
                             // clears shares_device_ok): the source stream may use the non-temporal policy
  bool shares_device_ok = true;
  gp_linearized6 view_store{};  // gp_vgicp_batch_linearize_view of a single large factor: the record the host combined from the finalize parts
  int ppt = 4;            // 64-point chunks per wave of the pipeline kernel (tile = 256 x ppt points)
  std::vector<gp::FactorDesc> h_descs;  // host copy of the factor table (a single factor rides in the kernel arguments)
  gp::PinnedArray h_poses;
  hipEvent_t h2d_done = nullptr;  // recorded behind every H2D copy of h_poses; the next staging waits on it
  gp::PinnedArray h_out;  // results land here straight from the finalize kernel (host-mapped, no D2H copy op)
  void* h_out_dev = nullptr;
  bool table_dirty = true;
  std::vector<uint64_t> seen;  // per factor: its generation + its target map's generation when the table was built
};

namespace gp {

// Tile-kernel families (GP_KERNEL_*, per batch: gp_vgicp_batch_set_tuning(GP_TUNE_KERNEL)):
//   GP_KERNEL_REFERENCE (0)   reference-shaped kernel (reference bucket table, one point per lane per stride, all modes): the in-library cross-check and
//                             the 92-sum path of non-orthonormal poses
//   GP_KERNEL_HASHED (2)      round-1/2 pipeline kernel over the hashed line table, f32 outer products: what a map without a block grid runs
//   GP_KERNEL_GRID_F64 (3)    round-2 pipeline kernel over the block grid, f64 throughout (parity 4e-10 / 1e-15 instead of 6e-9)
//   GP_KERNEL_LOOKAHEAD (8)   round-2 pipeline kernel, block grid, f32 outer products, look-ahead lookup: what maps with >= 2^26 voxels run
//   GP_KERNEL_STREAM (12)     third generation (gp_vgicp_stream.hpp): per-wave chunk streams, balanced single-factor launches, surface validation
//                             in the ring.  Default.
// A family that does not apply to a batch (no block grid, records beyond 32-bit offsets) falls back to LOOKAHEAD, and
// that to HASHED.  Measured and removed (numbers: DESIGN.md section 8 of rounds 1-3): the f64 hashed kernel, the non-lean start, forced 512- / 256-point
// tiles, the deep pipeline, the source-frame formulation.
// (the A/B switches of rounds 2-3 -- GP_POSES_ZERO_COPY, GP_FINALIZE_PARTS, GP_FINALIZE_NARROW, GP_FINALIZE_HOST_EXPAND: environment variables read once per
// process -- are gone: their measurements are in profiles/r02_*, r03_* and DESIGN.md; the winners are constants.  The library reads no environment variable that
// changes what it computes or launches.)
constexpr int kFinalizePartsMax = 16;
// workgroups sharing the finalize of a synchronous single-factor call (A/B on C2, scripts/r02/r02_finalize_parts.sh: 1: 7.1 us, 2: 5.5, 4: 4.8, 8: 4.6, 16: 4.7 and the host step suffers;
// round 4, fused form, 8 against 16: C2 fused kernel 12.2-12.8 vs 12.1-12.9 us, step 19.9-20.2 vs 20.0-20.6; 125 k points: kernel 6.4-6.5 vs 6.2, step 13.7-14.4 vs 14.2-14.7)
constexpr int kFinalizeParts = 8;
constexpr int kFinalizeSplitTiles = 256;  // ... when the factor has at least this many tiles

// where a launch takes its poses from
struct PoseSource {
  const double* d_lin = nullptr;
  const double* d_eval = nullptr;
  gp::InlinePoses inl{};
};

inline int partials_ptr(gp_vgicp_batch* b, double** out) {
  if (b->temp_buffer) {
    void* p = nullptr;
    GP_TRY(gp_temp_buffer_get(b->temp_buffer, sizeof(double) * gp::ACCG_STRIDE * (size_t)std::max(b->num_tiles, 1), &p));
    *out = reinterpret_cast<double*>(p);
  } else {
    *out = b->d_partials.as<double>();
  }
  return GP_OK;
}

// the launches (gp_vgicp.hip).  launch_tiles: MODE_LIN, MODE_ERR or MODE_LIN_GENERAL; launch_finalize: the rigid (29-sum) or the general (92-sum) rows.
// parts > 1: that many workgroups per factor, each a record of its share of the rows; parts < 0: |parts| workgroups that deliver their 32 sums (the host expands)
template <int MODE>
int launch_tiles(gp_vgicp_batch* b, const PoseSource& ps, double* partials);
template <bool GENERAL>
int launch_finalize(gp_vgicp_batch* b, const PoseSource& ps, const double* partials, gp_linearized6* out_dev, DoneFlags done = {}, int parts = 1);
int launch_linearize(gp_vgicp_batch* b, const PoseSource& ps, gp_linearized6* out_dev, bool rigid, DoneFlags done = {}, int parts = 1, bool timed = false);
int launch_error(gp_vgicp_batch* b, const PoseSource& ps, double* out_dev, DoneFlags done = {});
int launch_finalize_error_parts(hipStream_t stream, const double* partials, int num_rows, int rows_per_part, int parts, double* out_dev, int out_stride, DoneFlags done);
int launch_source_extent(hipStream_t stream, const float* points, long long count, unsigned* out);  // source_extent_kernel: largest |coordinate| of a cloud (measure_extents)

// what gp_vgicp_table.hip gives the entry-point units (not part of the library's interface)
#pragma GCC visibility push(hidden)
int apply_tuning(gp_vgicp_tuning* t, int key, int value);      // one settable GP_TUNE_* key of a factor's or a batch's tuning
bool read_tuning(const gp_vgicp_tuning& t, int key, int* value);  // ... and one readable key (false: not a readable key of the tuning)
int build_table(gp_vgicp_batch* b);
bool table_is_stale(const gp_vgicp_batch* b);
inline int ensure_table(gp_vgicp_batch* b) { return table_is_stale(b) ? build_table(b) : GP_OK; }
int ensure_self_batch(gp_vgicp_factor* f);  // the factor's batch of one, its table built
bool takes_rigid_path(const gp_vgicp_batch* b, const double* poses_host);
int stage_poses(gp_vgicp_batch* b, const double* lin, const double* eval, PoseSource* ps, bool zero_copy = false);
// the poses of a single factor in the kernel arguments (table built)
inline void inline_poses(const gp_vgicp_batch* b, const double* lin, const double* eval, PoseSource* ps) {
  memcpy(ps->inl.lin, lin, sizeof(double) * 16);
  if (eval) memcpy(ps->inl.eval, eval, sizeof(double) * 16);
  ps->inl.factor = b->h_descs[0];
  ps->inl.tile_points = b->tile_points;
  ps->inl.use = 1;
}
// ... and the poses of any batch in device tables (double[F][16] each; inl.use stays 0)
inline PoseSource device_poses(const double* lin_dev, const double* eval_dev = nullptr) {
  PoseSource ps;
  ps.d_lin = lin_dev, ps.d_eval = eval_dev;
  return ps;
}
// a single rigid factor of at least kFinalizeSplitTiles tiles shares its linearise's finalize among kFinalizeParts workgroups
inline int linearize_parts(const gp_vgicp_batch* b, bool rigid) {
  return (b->factors.size() == 1 && rigid && b->num_tiles >= kFinalizeSplitTiles) ? kFinalizeParts : 1;
}
#pragma GCC visibility pop

}  // namespace gp
